// pin.hip -- pin_pq / pin_ivf / pin_ivf_multi: the pinned tables' layouts in HBM; append_rows / remove_rows / update_rows / update_codebook.
#include "internal.h"

#include "kernels.h"
#include "scan_common.h"
#include "coarse.h"   // fragment layouts of the centroids; refine.h: row_term_kernel
#include "remove_kernels.h"
#include "update_kernels.h"

static std::vector<float> transpose_codebook(const float* cb, int m, int K, int S) {
  std::vector<float> t((size_t)m * S * K);
  for (int p = 0; p < m; ++p)
    for (int c = 0; c < K; ++c)
      for (int j = 0; j < S; ++j) t[((size_t)p * S + j) * K + c] = cb[((size_t)p * K + c) * S + j];
  return t;
}

// Pack rows of `n_lists` inverted lists into 64-row blocks: [block][M2][64] dwords, two
// int16 codes per dword, plus one scan-position dword per row (-1 on padding rows).
// Which rows share a 16-lane group of a 64-row block decides what the scan kernels' LDS gathers cost: a
// wave-level ds_read_b128 of slab rows takes ~2.4 + 4 x (largest number of lanes of a 16-lane group whose
// rows' codes agree modulo 16 = the same LDS bank group) cycles (tools/lab/ubench6: 14.6 cycles for random
// rows, 6.4 without collisions).  The order of the rows inside a list is free (results are ordered by id
// in the merge), so the rows of every group are picked greedily -- each next row from a window of 64
// candidates, the one that raises the per-position maxima least -- which brings the average maximum
// from 3.06 to ~2.1.  order[] = the list's rows in packing order.
static void arrange_list_rows(const int16_t* codes, int m, int64_t lo, int64_t hi, std::vector<int64_t>& order) {
  const int64_t n = hi - lo;
  order.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = lo + i;
  if (n <= 16 || m > 16) return;
  static const int WINDOW = (int)env_int("FREDDY_GPU_ARRANGE_WINDOW", 1024);   // candidates looked at for every pick (64: scan 103 us, 256: 101.7, 1024: 99.8; pin time 0.2 / 0.4 / 1.3 s for 3 M rows)
  int cnt[16][16], mx[16];
  for (int64_t k = 0; k < n; ++k) {
    if ((k & 15) == 0) { memset(cnt, 0, sizeof(cnt)); memset(mx, 0, sizeof(mx)); }
    const int64_t wend = std::min<int64_t>(n, k + WINDOW);
    int64_t best = k;
    int best_cost = INT32_MAX;
    for (int64_t j = k; j < wend; ++j) {
      const int16_t* row = codes + (size_t)order[(size_t)j] * m;
      int cost = 0;
      for (int p = 0; p < m; ++p) {
        const int c = cnt[p][row[p] & 15];
        cost += c + (c + 1 > mx[p] ? 100 : 0);
      }
      if (cost < best_cost) { best_cost = cost; best = j; }
    }
    std::swap(order[(size_t)k], order[(size_t)best]);
    const int16_t* row = codes + (size_t)order[(size_t)k] * m;
    for (int p = 0; p < m; ++p) {
      const int c = ++cnt[p][row[p] & 15];
      if (c > mx[p]) mx[p] = c;
    }
  }
  // The 16 rows picked together have to sit in the 16 lanes the LDS serves together -- and for ds_read_b128
  // those are NOT 16 consecutive lanes but {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32
  // (MI355X_MICROARCH.md, LDS).  (Round 1 placed each group in consecutive lanes: every hardware group then
  // mixed the halves of two picked groups, and the arrangement bought 2 % instead of what tools/lab/ubench6 promised.)
  static const int GROUP_LANES[64] = {0,  1,  2,  3,  12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27, 4,  5,  6,  7,  8,  9,
                                      10, 11, 16, 17, 18, 19, 28, 29, 30, 31, 32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55,
                                      56, 57, 58, 59, 36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63};
  std::vector<int64_t> blk(64);
  for (int64_t b0 = 0; b0 + 64 <= n; b0 += 64) {   // (a partial last block keeps its rows in the first lanes)
    for (int j = 0; j < 64; ++j) blk[(size_t)GROUP_LANES[j]] = order[(size_t)(b0 + j)];
    for (int j = 0; j < 64; ++j) order[(size_t)(b0 + j)] = blk[(size_t)j];
  }
}

static int pack_lists(freddy_gpu_index* ix, int n_lists, const int32_t* list_off, const int16_t* codes,
                      const int32_t* row_pos /*NULL: row index*/) {
  const int m = ix->m, K = ix->K, M2 = ix->M2;
  std::vector<int32_t> blk_off(n_lists + 1, 0);
  int max_blocks = 0;
  for (int c = 0; c < n_lists; ++c) {
    const int64_t len = (int64_t)list_off[c + 1] - list_off[c];
    if (len < 0) return fail(FREDDY_E_ARG, "list_off is not non-decreasing at list %d", c);
    const int nb = (int)((len + 63) / 64);
    blk_off[c + 1] = blk_off[c] + nb;
    max_blocks = std::max(max_blocks, nb);
  }
  const int64_t n_blocks = blk_off[n_lists];
  std::vector<uint32_t> packed((size_t)std::max<int64_t>(n_blocks, 1) * M2 * 64, 0u);
  std::vector<int32_t> pos((size_t)std::max<int64_t>(n_blocks, 1) * 64, -1);
  // (inverted lists only: the flat PQ table is addressed by row index)
  const bool arrange = row_pos != nullptr;
  std::vector<std::vector<int64_t>> orders(arrange ? (size_t)n_lists : 0);
  if (arrange) {
    std::atomic<int> next_list{0};
    auto worker = [&]() {
      for (int c = next_list.fetch_add(1); c < n_lists; c = next_list.fetch_add(1))
        arrange_list_rows(codes, m, list_off[c], list_off[c + 1], orders[(size_t)c]);
    };
    const unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt && (int)t < n_lists; ++t) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
  }
  for (int c = 0; c < n_lists; ++c) {
    for (int64_t i = 0; i < (int64_t)list_off[c + 1] - list_off[c]; ++i) {
      const int64_t r = arrange ? orders[(size_t)c][(size_t)i] : list_off[c] + i;
      const int64_t b = blk_off[c] + i / 64;
      const int lane = (int)(i % 64);
      const int16_t* row = codes + (size_t)r * m;
      for (int l = 0; l < m; ++l) {
        if (row[l] < 0 || row[l] >= K)
          return fail(FREDDY_E_ARG, "code %d at row %lld position %d is outside [0,%d)", (int)row[l],
                      (long long)r, l, K);
      }
      for (int j = 0; j < M2; ++j) {
        const uint32_t lo = (uint16_t)row[2 * j];
        const uint32_t hi = (2 * j + 1 < m) ? (uint16_t)row[2 * j + 1] : 0u;
        packed[((size_t)b * M2 + j) * 64 + lane] = lo | (hi << 16);
      }
      pos[(size_t)b * 64 + lane] = row_pos ? row_pos[r] : (int32_t)r;
    }
  }
  std::vector<int32_t> blk_cell((size_t)std::max<int64_t>(n_blocks, 1), 0);
  for (int c = 0; c < n_lists; ++c)
    for (int b = blk_off[c]; b < blk_off[c + 1]; ++b) blk_cell[(size_t)b] = c;
  if (upload(&ix->blk_cell, blk_cell.data(), blk_cell.size(), &ix->bytes))
    return fail(FREDDY_E_NOMEM, "device allocation/copy failed while pinning the lists");
  ix->n_blocks = n_blocks;
  ix->max_list_blocks = max_blocks;
  ix->h_list_off.assign(list_off, list_off + n_lists + 1);
  if (upload(&ix->blk_off, blk_off.data(), blk_off.size(), &ix->bytes) ||
      upload(&ix->list_off, list_off, (size_t)n_lists + 1, &ix->bytes) ||
      upload(&ix->packed, packed.data(), packed.size(), &ix->bytes) ||
      upload(&ix->pos, pos.data(), pos.size(), &ix->bytes))
    return fail(FREDDY_E_NOMEM, "device allocation/copy failed while pinning the lists");
  return 0;
}

// packed[block][6][64] (two int16 codes per dword) -> packed8[block][3][64] (four one-byte codes per dword)
__global__ __launch_bounds__(256) void pack8_kernel(const uint32_t* __restrict__ packed, uint32_t* __restrict__ packed8, int64_t n_blocks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (block, t, lane)
  if (i >= n_blocks * 3 * 64) return;
  const int lane = (int)(i & 63);
  const int64_t bt = i >> 6;
  const int t = (int)(bt % 3);
  const int64_t b = bt / 3;
  const uint32_t p0 = packed[((size_t)b * 6 + 2 * t) * 64 + lane], p1 = packed[((size_t)b * 6 + 2 * t + 1) * 64 + lane];
  packed8[i] = (p0 & 0xffu) | (((p0 >> 16) & 0xffu) << 8) | ((p1 & 0xffu) << 16) | (((p1 >> 16) & 0xffu) << 24);
}
// The one-byte code array of a block array `packed` of a handle whose codes fit a byte (K <= 256, m = 12: the cell-grouped scans'
// shape), built BESIDE whatever the handle holds: *out stays NULL (and *out_bytes 0) for every other shape.  The handle is not
// touched; a failure leaves nothing behind.  (Until the allocation seam a failed allocation here was swallowed -- "the int16
// layout serves" -- so that a handle could silently differ from a fresh pin of its table; now it is the call's failure.)
static int make_packed8(const freddy_gpu_index* ix, const uint32_t* packed, int64_t n_blocks, uint32_t** out, int64_t* out_bytes) {
  *out = nullptr; *out_bytes = 0;
  if (ix->K > 256 || ix->m != 12 || ix->M2 != 6 || !packed || n_blocks <= 0) return 0;
  const size_t bytes = sizeof(uint32_t) * (size_t)n_blocks * 3 * 64;
  if (dev_malloc(out, bytes) != hipSuccess) { *out = nullptr; return fail(FREDDY_E_NOMEM, "device allocation of %zu bytes failed (one-byte codes)", bytes); }
  const int64_t n = n_blocks * 3 * 64;
  hipLaunchKernelGGL(pack8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, packed, *out, n_blocks);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) {
    (void)dev_free(*out); *out = nullptr;
    return fail(FREDDY_E_HIP, "building the one-byte codes failed");
  }
  *out_bytes = (int64_t)bytes;
  return 0;
}
// the handle's array gives way to `p8` (NULL: none)
static void install_packed8(freddy_gpu_index* ix, uint32_t* p8, int64_t bytes) {
  if (ix->packed8 && ix->packed8_own) { (void)dev_free(ix->packed8); ix->bytes -= ix->packed8_bytes; }
  ix->packed8 = p8; ix->packed8_own = p8 != nullptr; ix->packed8_bytes = bytes;
  ix->bytes += bytes;
}
// (Re)build it from the handle's own block array (pin time; update_rows, which rewrites that array in place): the old copy stays
// until the new one is complete.
static int build_packed8(freddy_gpu_index* ix) {
  uint32_t* p8 = nullptr;
  int64_t bytes = 0;
  if (int rc = make_packed8(ix, ix->packed, ix->n_blocks, &p8, &bytes)) return rc;
  install_packed8(ix, p8, bytes);
  return 0;
}

// Everything on the device that is a function of the (residual) codebook: the transposed copy of the generic
// LUT kernel, the paired layout of the exact fused scan, and -- for the filter + refine scan -- the row-major
// copy and the norm bounds.  (Re)built at pin time and by freddy_gpu_update_codebook; the row terms follow
// in refresh_row_terms once the rows are in place.
// Everything that is derived from the codebook.  The new tables -- and, with rows in place (with_row_terms:
// freddy_gpu_update_codebook on a live ivf handle), the row terms that follow from them -- are built beside the old ones and
// swapped in only when every allocation, upload and launch has succeeded: a failed call leaves the handle as it was.
static int derive_codebook_tables_into(freddy_gpu_index* ix, const float* codebook);
static int make_row_terms(const freddy_gpu_index* ix, const uint32_t* packed, const int32_t* blk_cell, int64_t n_blocks, const float* cbR, float** out, int64_t* out_bytes);
static void install_row_terms(freddy_gpu_index* ix, float* rterm, int64_t bytes);
static int derive_codebook_tables(freddy_gpu_index* ix, const float* codebook, bool with_row_terms = false) {
  float* const old[] = {ix->cbT, ix->cbP, ix->cbR, ix->pmax, ix->cmaxp, ix->cbF};
  const int64_t bytes_before = ix->bytes;
  ix->cbT = ix->cbP = ix->cbR = ix->pmax = ix->cmaxp = ix->cbF = nullptr;
  int rc = derive_codebook_tables_into(ix, codebook);
  float* rterm = nullptr;
  int64_t rterm_bytes = 0;
  if (!rc && with_row_terms) rc = make_row_terms(ix, ix->packed, ix->blk_cell, ix->n_blocks, ix->cbR, &rterm, &rterm_bytes);
  if (rc) {   // put the old tables back
    float* const fresh[] = {ix->cbT, ix->cbP, ix->cbR, ix->pmax, ix->cmaxp, ix->cbF};
    for (float* p : fresh) if (p) (void)dev_free(p);
    ix->cbT = old[0]; ix->cbP = old[1]; ix->cbR = old[2]; ix->pmax = old[3]; ix->cmaxp = old[4]; ix->cbF = old[5];
    ix->bytes = bytes_before;
    return rc;
  }
  if (with_row_terms) install_row_terms(ix, rterm, rterm_bytes);
  int64_t old_bytes = 0;
  if (old[0]) old_bytes += (int64_t)sizeof(float) * ix->m * ix->S * ix->K;
  if (old[1]) old_bytes += (int64_t)sizeof(float) * ix->m * (((ix->S + 3) & ~3) / 4) * FUSED_T * 8;
  if (old[2]) old_bytes += (int64_t)sizeof(float) * ix->m * ix->K * ix->S;
  if (old[3]) old_bytes += (int64_t)sizeof(float) * ix->m;
  if (old[4]) old_bytes += (int64_t)sizeof(float) * ix->m;
  if (old[5]) old_bytes += (int64_t)sizeof(float) * ix->m * 8 * 7 * 64 * 8;
  ix->bytes -= old_bytes;       // (the footprint changes by the difference, not by a second copy)
  for (float* p : old) if (p) (void)dev_free(p);
  if (ix->kind == KIND_PQ) {    // views of the flat table are rebuilt from the new tables on next use
    if (ix->pq_shadow) { free_index(ix->pq_shadow); ix->pq_shadow = nullptr; }
    if (ix->pq_sub_view) { free_index(ix->pq_sub_view); ix->pq_sub_view = nullptr; }
  }
  return 0;
}
// The codebook in the order the table kernel's v_mfma_f32_16x16x4_f32 B operands are read (m = 12, S = 25, K <= 1024): for
// (position, group g of 16 code slots, step) lane l = (col = l & 15, kq = l >> 4) finds the eight values of dimension
// 4 step + kq for the codes 128 i + 16 g + col + 512 e, (i, e) = (0,0) (0,1) (1,0) ... (3,1), as two 16-byte words: a wave's
// load is 2 KB of consecutive bytes (the transposed copy gave 64-byte pieces of eight different lines).
static int build_fragment_codebook(freddy_gpu_index* ix, const float* codebook) {
  std::vector<float> f((size_t)ix->m * 8 * 7 * 64 * 8, 0.0f);
  for (int p = 0; p < ix->m; ++p)
    for (int g = 0; g < 8; ++g)
      for (int st = 0; st < 7; ++st)
        for (int l = 0; l < 64; ++l)
          for (int i = 0; i < 4; ++i)
            for (int e = 0; e < 2; ++e) {
              const int j = 4 * st + (l >> 4), c = 128 * i + 16 * g + (l & 15) + 512 * e;
              if (j < ix->S && c < ix->K)
                f[((((size_t)p * 8 + g) * 7 + st) * 64 + l) * 8 + i * 2 + e] = codebook[((size_t)p * ix->K + c) * ix->S + j];
            }
  if (upload(&ix->cbF, f.data(), f.size(), &ix->bytes)) return fail(FREDDY_E_NOMEM, "device allocation failed");
  return 0;
}
// The largest norm so far, a NaN included and kept: std::max drops a NaN operand, and the filter's margin E must turn non-finite
// when any codeword or centroid is (refine.h: every row then goes to the exact stage) -- a finite E over a table with a NaN in
// it emptied the lists of the queries whose smallest cheap distances came from the rows that use the NaN codeword.
static inline double norm_max(double a, double b) { return (b != b || b > a) ? b : a; }
static int derive_codebook_tables_into(freddy_gpu_index* ix, const float* codebook) {
  std::vector<float> cbT = transpose_codebook(codebook, ix->m, ix->K, ix->S);
  if (upload(&ix->cbT, cbT.data(), cbT.size(), &ix->bytes)) return fail(FREDDY_E_NOMEM, "device allocation failed");
  if (ix->kind == KIND_PQ) {
    // batches over the flat table take the cell-grouped filter + refine scan (pq_shadow_build): its codebook-derived tables,
    // with "centroids" that are zero
    if (ix->m == 12 && ix->S == 25 && ix->K <= FUSED_T * FUSED_E) {
      std::vector<float> cmaxp((size_t)ix->m);
      for (int p = 0; p < ix->m; ++p) {
        double cmax = 0.0;
        for (int c = 0; c < ix->K; ++c) {
          double n2 = 0.0;
          for (int j = 0; j < ix->S; ++j) { const double v = codebook[((size_t)p * ix->K + c) * ix->S + j]; n2 += v * v; }
          cmax = norm_max(cmax, std::sqrt(n2));
        }
        cmaxp[p] = (float)(cmax * (1.0 + 1e-6));
      }
      if (upload(&ix->cbR, codebook, (size_t)ix->m * ix->K * ix->S, &ix->bytes) ||
          upload(&ix->pmax, cmaxp.data(), cmaxp.size(), &ix->bytes) ||
          upload(&ix->cmaxp, cmaxp.data(), cmaxp.size(), &ix->bytes))
        return fail(FREDDY_E_NOMEM, "device allocation failed");
      if (int rc = build_fragment_codebook(ix, codebook)) return rc;
    }
    return 0;
  }
  if (ix->kind != KIND_IVF) return 0;
  const int C = ix->C, d = ix->d;
  if (ix->K <= FUSED_T * FUSED_E) {
    // paired layout of the fused kernels: slot t holds codes (t, t+512); 4 dims x 2 codes per 32 bytes.
    // (Splitting the two 16-byte halves of a slot into separate contiguous arrays measured SLOWER: the
    // second load of a slot then no longer hits the lines the first one brought in.)
    const int SP = (ix->S + 3) & ~3, SPq = SP / 4;
    std::vector<float> cbP((size_t)ix->m * SPq * FUSED_T * 8, 0.0f);
    for (int p = 0; p < ix->m; ++p)
      for (int jb = 0; jb < SPq; ++jb)
        for (int tl = 0; tl < FUSED_T; ++tl)
          for (int u = 0; u < 4; ++u)
            for (int e = 0; e < 2; ++e) {
              const int j = jb * 4 + u, c = tl + e * FUSED_T;
              if (j < ix->S && c < ix->K)
                cbP[((((size_t)p * SPq + jb) * FUSED_T + tl) * 4 + u) * 2 + e] = codebook[((size_t)p * ix->K + c) * ix->S + j];
            }
    if (upload(&ix->cbP, cbP.data(), cbP.size(), &ix->bytes)) return fail(FREDDY_E_NOMEM, "device allocation failed");
  }
  // filter + refine tables (refine.h)
  if (ix->cbP && ix->m == 12 && ix->S == 25) {
    std::vector<float> pmax((size_t)ix->m), cmaxp((size_t)ix->m);
    for (int p = 0; p < ix->m; ++p) {
      double comax = 0.0, cmax = 0.0;
      for (int c = 0; c < C; ++c) {
        double n2 = 0.0;
        for (int j = 0; j < ix->S; ++j) { const double v = ix->h_coarse[(size_t)c * d + p * ix->S + j]; n2 += v * v; }
        comax = norm_max(comax, std::sqrt(n2));
      }
      for (int c = 0; c < ix->K; ++c) {
        double n2 = 0.0;
        for (int j = 0; j < ix->S; ++j) { const double v = codebook[((size_t)p * ix->K + c) * ix->S + j]; n2 += v * v; }
        cmax = norm_max(cmax, std::sqrt(n2));
      }
      pmax[p] = (float)((comax + cmax) * (1.0 + 1e-6));
      cmaxp[p] = (float)(cmax * (1.0 + 1e-6));
    }
    if (upload(&ix->cbR, codebook, (size_t)ix->m * ix->K * ix->S, &ix->bytes) ||
        upload(&ix->pmax, pmax.data(), pmax.size(), &ix->bytes) ||
        upload(&ix->cmaxp, cmaxp.data(), cmaxp.size(), &ix->bytes))
      return fail(FREDDY_E_NOMEM, "device allocation failed");
    if (int rc = build_fragment_codebook(ix, codebook)) return rc;
  }
  return 0;
}

// rterm[slot] for every row slot of the lists `packed` / `blk_cell` (the (cell, row) part of the filter's cheap distance) under the
// row-major codebook cbR, built BESIDE what the handle holds: *out stays NULL without cbR (no filter + refine tables).  The handle
// is not touched; a failure leaves nothing behind.
static int make_row_terms(const freddy_gpu_index* ix, const uint32_t* packed, const int32_t* blk_cell, int64_t n_blocks, const float* cbR, float** out, int64_t* out_bytes) {
  *out = nullptr; *out_bytes = 0;
  if (!cbR) return 0;
  const int64_t n_slots = std::max<int64_t>(n_blocks, 1) * 64;
  if (dev_malloc(out, sizeof(float) * (size_t)n_slots) != hipSuccess) { *out = nullptr; return fail(FREDDY_E_NOMEM, "device allocation failed (row terms)"); }
  if (n_blocks > 0) {
    hipLaunchKernelGGL(row_term_kernel, dim3((unsigned)((n_blocks * 64 + 255) / 256)), dim3(256), 0, ix->stream, packed,
                       blk_cell, ix->coarse, cbR, *out, n_blocks * 64, ix->M2, ix->d, ix->m, ix->K, ix->S);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) {
      (void)dev_free(*out); *out = nullptr;
      return fail(FREDDY_E_HIP, "building the row terms failed");
    }
  }
  *out_bytes = (int64_t)sizeof(float) * n_slots;
  return 0;
}
// the handle's row terms give way to `rterm` (NULL: none)
static void install_row_terms(freddy_gpu_index* ix, float* rterm, int64_t bytes) {
  if (ix->rterm) (void)dev_free(ix->rterm);
  ix->bytes += bytes - ix->rterm_bytes;
  ix->rterm = rterm; ix->rterm_bytes = bytes;
}
// from the handle's own arrays (pin time; update_rows, which rewrites them in place): the old terms stay until the new ones are complete
static int refresh_row_terms(freddy_gpu_index* ix) {
  float* rterm = nullptr;
  int64_t bytes = 0;
  if (int rc = make_row_terms(ix, ix->packed, ix->blk_cell, ix->n_blocks, ix->cbR, &rterm, &bytes)) return rc;
  install_row_terms(ix, rterm, bytes);
  return 0;
}

static int raise_lds_limits(int device) {
  static std::mutex mu;
  static std::vector<char> done;
  std::lock_guard<std::mutex> g(mu);
  if ((size_t)device < done.size() && done[(size_t)device]) return 0;
  for (const std::vector<LdsLimit>& unit : {lds_limits_ivfadc(), lds_limits_pq(), lds_limits_join(), lds_limits_exact()})
    for (const LdsLimit& l : unit) HIP_TRY(hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, l.bytes));
  if (done.size() <= (size_t)device) done.resize((size_t)device + 1, 0);
  done[(size_t)device] = 1;
  return 0;
}

int open_device(freddy_gpu_index* ix, int device) {
  // The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), read once when the
  // runtime starts: the pipeline's four lanes want a queue each beside the library's own stream (6 queues measured
  // best for ONE process) -- but several backends with six queues each are together slower than one, so a process that
  // finds other live backends takes two (core.hip choose_hw_queues).  Never overrides the environment; without effect if
  // the runtime is already up.
  // (the registry counts backends per PHYSICAL GPU: one process per GPU -- bench.py --gpus N, one PostgreSQL cluster per GPU -- are not neighbours)
  if (!ix->registered) { ix->registered = true; backend_handles(+1, device); }   // (before the count of the others: two backends that start together see each other)
  choose_hw_queues(device);
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(FREDDY_E_ARG, "device %d out of range (%d visible)", device, n);
  HIP_TRY(hipSetDevice(device));
  ix->device = device;
  ix->tune = read_tuning();
  if (int rc = raise_lds_limits(device)) return rc;
  HIP_TRY(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ix->n_cus = prop.multiProcessorCount;
  return 0;
}

static int check_pq_shape(int d, int m, int K, int64_t N) {
  if (d <= 0 || m <= 0 || K <= 0 || N < 0) return fail(FREDDY_E_ARG, "non-positive dimension");
  if (d % m) return fail(FREDDY_E_ARG, "d=%d is not a multiple of m=%d", d, m);
  if (K > 65536) return fail(FREDDY_E_LIMIT, "K=%d does not fit a 16-bit code", K);
  if ((size_t)m * K * 4 + 4096 > 160 * 1024)
    return fail(FREDDY_E_LIMIT, "LUT of m*K=%d floats does not fit the 160 KiB LDS", m * K);
  if (N > (int64_t)INT32_MAX - 64) return fail(FREDDY_E_LIMIT, "N too large for 32-bit row positions");
  return 0;
}

extern "C" int freddy_gpu_pin_pq(const freddy_pq_desc* t, int device, freddy_gpu_index_t** out) {
  if (!t || !out || !t->codebook || (t->N && (!t->ids || !t->codes))) return fail(FREDDY_E_ARG, "NULL argument");
  if (int rc = check_pq_shape(t->d, t->m, t->K, t->N)) return rc;
  for (int64_t r = 1; r < t->N; ++r)
    if (t->ids[r] <= t->ids[r - 1])
      return fail(FREDDY_E_ARG, "ids must be strictly ascending (canonical scan order); violated at row %lld", (long long)r);
  freddy_gpu_index* ix = new freddy_gpu_index();
  ix->kind = KIND_PQ;
  ix->d = t->d; ix->m = t->m; ix->K = t->K; ix->S = t->d / t->m; ix->M2 = (t->m + 1) / 2; ix->N = t->N;
  int rc = open_device(ix, device);
  if (!rc) rc = derive_codebook_tables(ix, t->codebook);
  if (!rc && upload(&ix->ids, t->ids, (size_t)t->N, &ix->bytes)) rc = fail(FREDDY_E_NOMEM, "device allocation failed");
  if (!rc) {
    const int32_t off[2] = {0, (int32_t)t->N};
    rc = pack_lists(ix, 1, off, t->codes, nullptr);
    if (!rc) rc = build_packed8(ix);
  }
  if (!rc) { ix->h_ids.assign(t->ids, t->ids + t->N); ix->max_id = t->N ? t->ids[t->N - 1] : -1; }
  if (rc) { free_index(ix); return rc; }
  *out = ix;
  return FREDDY_OK;
}

extern "C" int freddy_gpu_pin_ivf(const freddy_ivf_desc* t, int device, freddy_gpu_index_t** out) {
  if (!t || !out || !t->codebook || !t->coarse || !t->list_off || (t->N && (!t->ids || !t->codes)))
    return fail(FREDDY_E_ARG, "NULL argument");
  if (int rc = check_pq_shape(t->d, t->m, t->K, t->N)) return rc;
  if (t->C <= 0) return fail(FREDDY_E_ARG, "C must be positive");
  // (coarse_dist_kernel, batches below 32 queries over vectors of more than 1024 dimensions: 16 queries of d floats in LDS)
  if ((size_t)t->d * 16 * sizeof(float) > 160 * 1024) return fail(FREDDY_E_LIMIT, "d=%d exceeds the IVFADC search's limit of 2560 dimensions", t->d);
  if (t->list_off[0] != 0 || t->list_off[t->C] != t->N) return fail(FREDDY_E_ARG, "list_off must span [0, N]");
  for (int c = 0; c < t->C; ++c)   // every offset is checked BEFORE any row is touched through it
    if (t->list_off[c] < 0 || t->list_off[c] > t->list_off[c + 1] || (int64_t)t->list_off[c + 1] > t->N)
      return fail(FREDDY_E_ARG, "list_off is not non-decreasing inside [0, N] at list %d", c);
  for (int c = 0; c < t->C; ++c)
    for (int64_t r = t->list_off[c]; r < t->list_off[c + 1]; ++r) {
      if (t->ids[r] < 0) return fail(FREDDY_E_ARG, "negative id at row %lld", (long long)r);
      if (r > t->list_off[c] && t->ids[r] <= t->ids[r - 1])
        return fail(FREDDY_E_ARG, "ids must be strictly ascending inside list %d (row %lld)", c, (long long)r);
    }
  {   // "unique overall": a row id may sit in one list only (the merge orders a query's candidates by id)
    std::vector<int32_t> sorted_ids(t->ids, t->ids + t->N);
    std::sort(sorted_ids.begin(), sorted_ids.end());
    for (int64_t r = 1; r < t->N; ++r)
      if (sorted_ids[(size_t)r] == sorted_ids[(size_t)r - 1])
        return fail(FREDDY_E_ARG, "id %d occurs in more than one list", (int)sorted_ids[(size_t)r]);
  }
  freddy_gpu_index* ix = new freddy_gpu_index();
  ix->kind = KIND_IVF;
  ix->d = t->d; ix->m = t->m; ix->K = t->K; ix->S = t->d / t->m; ix->M2 = (t->m + 1) / 2; ix->N = t->N; ix->C = t->C;
  int rc = open_device(ix, device);
  if (!rc) {
    ix->Cpad = (t->C + WG - 1) / WG * WG;
    std::vector<float> cT((size_t)t->d * ix->Cpad, 0.0f);
    for (int c = 0; c < t->C; ++c)
      for (int i = 0; i < t->d; ++i) cT[(size_t)i * ix->Cpad + c] = t->coarse[(size_t)c * t->d + i];
    if (upload(&ix->coarse, t->coarse, (size_t)t->C * t->d, &ix->bytes) ||
        upload(&ix->coarseT, cT.data(), cT.size(), &ix->bytes))
      rc = fail(FREDDY_E_NOMEM, "device allocation failed");
    if (!rc) {   // MFMA coarse kernel (coarse.h): zero-padded rows, squared norms (fp64, rounded once), largest norm
      ix->dp = (t->d + COARSE_DP_ALIGN - 1) / COARSE_DP_ALIGN * COARSE_DP_ALIGN;
      // fragment order [Cpad / 32][dp / 8][lane = 32 h + r][4]: element t = c[32 g + r][8 i + 4 h + t]
      std::vector<float> cP((size_t)ix->Cpad * ix->dp, 0.0f), cn2((size_t)ix->Cpad, 0.0f);
      const int nit = ix->dp / 8;
      double cmax2 = 0.0;
      for (int c = 0; c < t->C; ++c) {
        double n2 = 0.0;
        for (int i = 0; i < t->d; ++i) {
          const float v = t->coarse[(size_t)c * t->d + i];
          const int it = i >> 3, hh = (i >> 2) & 1, tt = i & 3;
          cP[((((size_t)(c >> 5) * nit + it) * 64) + (size_t)hh * 32 + (c & 31)) * 4 + tt] = v;
          n2 += (double)v * (double)v;
        }
        cn2[(size_t)c] = (float)n2;
        cmax2 = std::max(cmax2, n2);
      }
      ix->cmax = (float)(std::sqrt(cmax2) * (1.0 + 1e-6));
      // the f16-split copy of the centroids for the matrix cores (coarse.h coarse_approx16_body; FREDDY_GPU_COARSE_H16=0: the fp32 tiles).
      // Many cells: the fp32 tiles are bound by the matrix pipe (134 -> 102 us at 13 000 cells); 1000 cells: 32 -> 29 us alone,
      // 54 -> 46 us with four batches in flight (fewer matrix-pipe cycles beside the other batches' kernels)
      if (env_int("FREDDY_GPU_COARSE_H16", 1) != 0 && t->d % 4 == 0) {
        float amax = 0.0f;
        for (size_t i = 0; i < (size_t)t->C * t->d; ++i) amax = std::max(amax, std::fabs(t->coarse[i]));
        int e = 0;
        if (amax > 0.0f && amax < 3e38f) { (void)frexpf(amax, &e); e = 14 - e; }
        ix->coarse_ec = e;
        const int T = (t->d + 15) / 16;
        std::vector<_Float16> cH((size_t)ix->Cpad * T * 2 * 8 * 2, (_Float16)0.0f);   // [Cpad/32][T][2][64][8]
        for (int c = 0; c < t->C; ++c)
          for (int i = 0; i < t->d; ++i) {
            const float v = ldexpf(t->coarse[(size_t)c * t->d + i], e);
            const _Float16 hi = (_Float16)v;
            const _Float16 lo = (_Float16)(v - (float)hi);
            const int tt = i >> 4, g = (i >> 3) & 1, u = i & 7;
            const size_t base = (((size_t)(c >> 5) * T + tt) * 2) * 64;
            cH[(base + (size_t)g * 32 + (c & 31)) * 8 + u] = hi;
            cH[(base + 64 + (size_t)g * 32 + (c & 31)) * 8 + u] = lo;
          }
        _Float16* dH = nullptr;
        if (upload(&dH, cH.data(), cH.size(), &ix->bytes)) rc = fail(FREDDY_E_NOMEM, "device allocation failed");
        ix->coarseH = dH;
      }
      if (rc) {} else
      if (upload(&ix->coarseP, cP.data(), cP.size(), &ix->bytes) || upload(&ix->cn2, cn2.data(), cn2.size(), &ix->bytes) ||
          dev_malloc((void**)&ix->viol, 256) != hipSuccess || hipMemset(ix->viol, 0, 256) != hipSuccess)
        rc = fail(FREDDY_E_NOMEM, "device allocation failed");
      else ix->elastic = ix->viol + 32;   // the elastic scan's four words (internal.h): bytes 128..143 of the same allocation, a 64-byte line of their own
    }
    if (!rc) { ix->h_coarse.assign(t->coarse, t->coarse + (size_t)t->C * t->d); rc = derive_codebook_tables(ix, t->codebook); }
  }
  if (!rc) rc = pack_lists(ix, t->C, t->list_off, t->codes, t->ids);
  if (!rc) rc = build_packed8(ix);
  if (!rc) rc = refresh_row_terms(ix);   // one float per row slot: the (cell, row) part of the filter's cheap distance
  if (!rc)
    for (int64_t r = 0; r < t->N; ++r) ix->max_id = std::max(ix->max_id, t->ids[r]);
  if (rc) { free_index(ix); return rc; }
  *out = ix;
  return FREDDY_OK;
}

extern "C" int freddy_gpu_pin_ivf_multi(const freddy_ivf_desc* t, const int* devices, int n_devices, freddy_gpu_index_t** out) {
  if (!devices || n_devices < 1 || !out) return fail(FREDDY_E_ARG, "bad device list");
  freddy_gpu_index* first = nullptr;
  if (int rc = freddy_gpu_pin_ivf(t, devices[0], &first)) return rc;
  for (int g = 1; g < n_devices; ++g) {
    freddy_gpu_index* rep = nullptr;
    if (int rc = freddy_gpu_pin_ivf(t, devices[g], &rep)) { free_index(first); return rc; }
    first->replicas.push_back(rep);
  }
  (void)hipSetDevice(devices[0]);
  *out = first;
  return FREDDY_OK;
}
// ---------------------------------------------------------------------------------------
// insert_batch: HBM index mutation
// ---------------------------------------------------------------------------------------
// new block j of list blk_cell[b] <- old block j of that list (or empty)
__global__ __launch_bounds__(256) void repack_blocks_kernel(const uint32_t* __restrict__ old_packed, const int32_t* __restrict__ old_pos,
                                                           const int32_t* __restrict__ old_blk_off, const int32_t* __restrict__ new_blk_off,
                                                           const int32_t* __restrict__ new_blk_cell, uint32_t* __restrict__ packed,
                                                           int32_t* __restrict__ pos, int64_t n_new_blocks, int M2) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= n_new_blocks) return;
  const int c = new_blk_cell[b];
  const int j = (int)(b - new_blk_off[c]);
  const bool have = j < old_blk_off[c + 1] - old_blk_off[c];
  const int64_t ob = (int64_t)old_blk_off[c] + j;
  for (int w = 0; w < M2; ++w) packed[((size_t)b * M2 + w) * 64 + lane] = have ? old_packed[((size_t)ob * M2 + w) * 64 + lane] : 0u;
  pos[(size_t)b * 64 + lane] = have ? old_pos[(size_t)ob * 64 + lane] : -1;
}
// new rows into their slots: slot[i] = row slot (block * 64 + lane) of new row i
__global__ __launch_bounds__(256) void place_rows_kernel(const int64_t* __restrict__ slot, const int32_t* __restrict__ row_pos,
                                                        const int16_t* __restrict__ codes, int64_t n, uint32_t* __restrict__ packed,
                                                        int32_t* __restrict__ pos, int m, int M2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t sl = slot[i], b = sl >> 6;
  const int lane = (int)(sl & 63);
  for (int w = 0; w < M2; ++w) {
    const uint32_t lo = (uint16_t)codes[(size_t)i * m + 2 * w];
    const uint32_t hi = (2 * w + 1 < m) ? (uint16_t)codes[(size_t)i * m + 2 * w + 1] : 0u;
    packed[((size_t)b * M2 + w) * 64 + lane] = lo | (hi << 16);
  }
  pos[(size_t)sl] = row_pos[i];
}
// raw vectors into the 64-row blocked layout: row r -> xb[r / 64][dim][r % 64]
__global__ __launch_bounds__(256) void place_vectors_kernel(const float* __restrict__ src, int64_t first_row, int64_t n, float* __restrict__ xb, int d) {
  const int64_t i = (int64_t)blockIdx.x;
  if (i >= n) return;
  const int64_t r = first_row + i;
  for (int dim = threadIdx.x; dim < d; dim += 256) xb[((r >> 6) * d + dim) * 64 + (r & 63)] = src[(size_t)i * d + dim];
}

// A longer copy of a device array BESIDE it: the old_n elements of `arr`, then append_n elements from the host.  *fresh is the
// caller's to swap in (swap_grown) or free; -1: no memory, -2: a copy failed -- nothing is left behind either way.
template <class T>
static int grown_copy(const T* arr, size_t old_n, size_t new_n, const T* append_host, size_t append_n, T** fresh) {
  *fresh = nullptr;
  if (dev_malloc(fresh, sizeof(T) * std::max<size_t>(new_n, 1)) != hipSuccess) { *fresh = nullptr; return -1; }
  if ((old_n && hipMemcpy(*fresh, arr, sizeof(T) * old_n, hipMemcpyDeviceToDevice) != hipSuccess) ||
      (append_n && hipMemcpy(*fresh + old_n, append_host, sizeof(T) * append_n, hipMemcpyHostToDevice) != hipSuccess)) {
    (void)dev_free(*fresh); *fresh = nullptr;
    return -2;
  }
  return 0;
}
template <class T>
static void swap_grown(T** arr, size_t old_n, size_t new_n, T* fresh, int64_t* bytes) {
  // (the footprint as upload() counts it: an empty array is one element)
  *bytes += (int64_t)(sizeof(T) * std::max<size_t>(new_n, 1)) - (*arr ? (int64_t)(sizeof(T) * std::max<size_t>(old_n, 1)) : 0);
  if (*arr) (void)dev_free(*arr);
  *arr = fresh;
}
static int grow_failed(int rc) { return rc == -1 ? fail(FREDDY_E_NOMEM, "device allocation failed while appending rows") : fail(FREDDY_E_HIP, "copying the rows failed"); }

// The arrays of a pq / ivf handle that follow its rows -- the block layout, the one-byte codes and (ivf) the row terms -- as
// append_packed_rows / remove_packed_rows build them BESIDE the pinned ones.  install_layout swaps them in, and only then does the
// handle change; what is never installed is freed when the record goes out of scope.  So a call that fails before install_layout
// leaves the handle as it was.
struct FreshLayout {
  uint32_t *packed = nullptr, *packed8 = nullptr;
  int32_t *pos = nullptr, *blk_cell = nullptr, *blk_off = nullptr, *list_off = nullptr;
  float* rterm = nullptr;
  int64_t packed8_bytes = 0, rterm_bytes = 0;
  int64_t n_blocks = 0, N = 0;
  int max_list_blocks = 0;
  std::vector<int32_t> h_list_off;
  bool ready = false;      // complete: install_layout may run (false after a call that found nothing to change)
  void drop() {
    void* all[] = {packed, packed8, pos, blk_cell, blk_off, list_off, rterm};
    for (void* p : all) if (p) (void)dev_free(p);
    packed = packed8 = nullptr; pos = blk_cell = blk_off = list_off = nullptr; rterm = nullptr;
    ready = false;
  }
  ~FreshLayout() { drop(); }
};
// what follows from the fresh block arrays: the one-byte codes, and the row terms of an ivf handle
static int finish_layout(freddy_gpu_index* ix, FreshLayout& L) {
  int rc = 0;
  if (!ix->shadow_of) rc = make_packed8(ix, L.packed, L.n_blocks, &L.packed8, &L.packed8_bytes);
  if (!rc && ix->kind == KIND_IVF) rc = make_row_terms(ix, L.packed, L.blk_cell, L.n_blocks, ix->cbR, &L.rterm, &L.rterm_bytes);
  if (rc) L.drop(); else L.ready = true;
  return rc;
}
static void install_layout(freddy_gpu_index* ix, FreshLayout& L) {
  void* old[] = {ix->packed, ix->pos, ix->blk_cell, ix->blk_off, ix->list_off};
  for (void* p : old) if (p) (void)dev_free(p);
  {   // the footprint follows the block count (pack_lists counts packed, pos and blk_cell with one block at least; blk_off and list_off keep their size)
    const int64_t ob = std::max<int64_t>(ix->n_blocks, 1), nb = std::max<int64_t>(L.n_blocks, 1);
    ix->bytes += (nb - ob) * (int64_t)(sizeof(uint32_t) * ix->M2 * 64 + sizeof(int32_t) * 64 + sizeof(int32_t));
  }
  ix->packed = L.packed; ix->pos = L.pos; ix->blk_cell = L.blk_cell; ix->blk_off = L.blk_off; ix->list_off = L.list_off;
  ix->n_blocks = L.n_blocks;
  ix->max_list_blocks = L.max_list_blocks;
  ix->h_list_off.swap(L.h_list_off);
  ix->N = L.N;
  if (!ix->shadow_of) install_packed8(ix, L.packed8, L.packed8_bytes);
  if (ix->kind == KIND_IVF) install_row_terms(ix, L.rterm, L.rterm_bytes);
  L.packed = L.packed8 = nullptr; L.pos = L.blk_cell = L.blk_off = L.list_off = nullptr; L.rterm = nullptr;
  L.ready = false;
}

// rows of a pq / ivf index: each new row goes to the end of its list; the 64-row block layout is rebuilt on
// the device (old blocks copied to their new places, new rows written into the free slots behind them) into L; the handle is
// not touched
static int append_packed_rows(freddy_gpu_index* ix, int n_lists, int64_t n, const int32_t* cell, const int32_t* row_pos, const int16_t* codes, FreshLayout& L) {
  const int m = ix->m, M2 = ix->M2;
  std::vector<int32_t> new_list_off((size_t)n_lists + 1, 0), add((size_t)n_lists, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int c = cell ? cell[i] : 0;
    if (c < 0 || c >= n_lists) return fail(FREDDY_E_ARG, "coarse_id %d of new row %lld is outside [0, %d)", c, (long long)i, n_lists);
    for (int l = 0; l < m; ++l)
      if (codes[(size_t)i * m + l] < 0 || codes[(size_t)i * m + l] >= ix->K)
        return fail(FREDDY_E_ARG, "code %d of new row %lld is outside [0, %d)", (int)codes[(size_t)i * m + l], (long long)i, ix->K);
    add[(size_t)c]++;
  }
  std::vector<int32_t> old_blk((size_t)n_lists + 1, 0), new_blk((size_t)n_lists + 1, 0);
  int max_blocks = 0;
  for (int c = 0; c < n_lists; ++c) {
    const int64_t old_len = ix->h_list_off[(size_t)c + 1] - ix->h_list_off[(size_t)c];
    old_blk[(size_t)c + 1] = old_blk[(size_t)c] + (int32_t)((old_len + 63) / 64);
    const int64_t len = old_len + add[(size_t)c];
    if ((int64_t)new_list_off[(size_t)c] + len > INT32_MAX - 64) return fail(FREDDY_E_LIMIT, "N too large for 32-bit row positions");
    new_list_off[(size_t)c + 1] = new_list_off[(size_t)c] + (int32_t)len;
    const int nb = (int)((len + 63) / 64);
    new_blk[(size_t)c + 1] = new_blk[(size_t)c] + nb;
    max_blocks = std::max(max_blocks, nb);
  }
  const int64_t n_new_blocks = new_blk[(size_t)n_lists];
  std::vector<int32_t> blk_cell((size_t)std::max<int64_t>(n_new_blocks, 1), 0);
  for (int c = 0; c < n_lists; ++c)
    for (int b = new_blk[(size_t)c]; b < new_blk[(size_t)c + 1]; ++b) blk_cell[(size_t)b] = c;
  std::vector<int64_t> slot((size_t)n);
  std::vector<int32_t> cursor((size_t)n_lists, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int c = cell ? cell[i] : 0;
    const int64_t old_len = ix->h_list_off[(size_t)c + 1] - ix->h_list_off[(size_t)c];
    slot[(size_t)i] = (int64_t)new_blk[(size_t)c] * 64 + old_len + cursor[(size_t)c]++;
  }
  uint32_t* packed = nullptr;
  int32_t *pos = nullptr, *d_blk_cell = nullptr, *d_new_blk = nullptr, *d_list_off = nullptr, *d_row_pos = nullptr;
  int64_t* d_slot = nullptr;
  int16_t* d_codes = nullptr;
  int64_t junk = 0;
  int rc = 0;
  if (dev_malloc((void**)&packed, sizeof(uint32_t) * (size_t)std::max<int64_t>(n_new_blocks, 1) * M2 * 64) != hipSuccess ||
      dev_malloc((void**)&pos, sizeof(int32_t) * (size_t)std::max<int64_t>(n_new_blocks, 1) * 64) != hipSuccess ||
      upload(&d_blk_cell, blk_cell.data(), blk_cell.size(), &junk) || upload(&d_new_blk, new_blk.data(), new_blk.size(), &junk) ||
      upload(&d_list_off, new_list_off.data(), new_list_off.size(), &junk) || upload(&d_slot, slot.data(), slot.size(), &junk) ||
      upload(&d_row_pos, row_pos, (size_t)n, &junk) || upload(&d_codes, codes, (size_t)n * m, &junk))
    rc = fail(FREDDY_E_NOMEM, "device allocation failed while appending rows");
  if (!rc && n_new_blocks > 0) {
    hipLaunchKernelGGL(repack_blocks_kernel, dim3((unsigned)((n_new_blocks + 3) / 4)), dim3(256), 0, ix->stream, ix->packed, ix->pos, ix->blk_off,
                       d_new_blk, d_blk_cell, packed, pos, n_new_blocks, M2);
    if (n > 0)
      hipLaunchKernelGGL(place_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, d_slot, d_row_pos, d_codes, n, packed, pos, m, M2);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "re-blocking the lists failed");
  }
  void* tmp[] = {d_slot, d_row_pos, d_codes};
  for (void* p : tmp) if (p) (void)dev_free(p);
  L.packed = packed; L.pos = pos; L.blk_cell = d_blk_cell; L.blk_off = d_new_blk; L.list_off = d_list_off;   // (L frees them if it is never installed)
  if (rc) { L.drop(); return rc; }
  L.n_blocks = n_new_blocks;
  L.max_list_blocks = max_blocks;
  L.h_list_off = new_list_off;
  L.N = ix->N + n;
  return finish_layout(ix, L);
}

extern "C" int freddy_gpu_append_rows(freddy_gpu_index_t* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id,
                                      const int16_t* codes, const float* vectors) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (n < 0 || (n > 0 && !ids)) return fail(FREDDY_E_ARG, "bad argument");
  if (n == 0) return FREDDY_OK;
  if (!ix->replicas.empty()) {
    // every replica holds the same tables: the primary goes first (argument errors are found there before anything has
    // changed anywhere); a failure after that leaves the devices with different tables -> the handle is poisoned and
    // every search on it fails loudly until it is unpinned
    std::vector<freddy_gpu_index*> reps;
    reps.swap(ix->replicas);
    int rc = freddy_gpu_append_rows(ix, n, ids, coarse_id, codes, vectors);
    reps.swap(ix->replicas);
    if (rc) return rc;   // (the primary is as it was, or has poisoned itself: no other device has changed)
    for (freddy_gpu_index* r : ix->replicas)
      if ((rc = freddy_gpu_append_rows(r, n, ids, coarse_id, codes, vectors))) { ix->poisoned = true; return rc; }
    return FREDDY_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  if (ix->kind == KIND_IVPQ) ix->join.tl_valid = false;   // (the cached "id IN (targets)" resolution refers to the rows as they were)
  const int32_t last_id = ix->kind == KIND_IVPQ ? (ix->join.h_ids.empty() ? -1 : ix->join.h_ids.back())
                          : ix->kind == KIND_IVF ? ix->max_id : (ix->h_ids.empty() ? -1 : ix->h_ids.back());
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] <= (i ? ids[i - 1] : last_id))
      return fail(FREDDY_E_ARG, "appended ids must ascend beyond the largest pinned id %d (row %lld has %d)", last_id, (long long)i, ids[i]);
  if (ix->N + n > (int64_t)INT32_MAX - 64) return fail(FREDDY_E_LIMIT, "N too large for 32-bit row positions");
  switch (ix->kind) {
    case KIND_PQ: {
      if (!codes) return fail(FREDDY_E_ARG, "codes are required");
      std::vector<int32_t> row_pos((size_t)n);
      for (int64_t i = 0; i < n; ++i) row_pos[(size_t)i] = (int32_t)(ix->N + i);   // flat table: position = row index
      const int64_t old_n = ix->N;
      // everything is built beside the pinned arrays; the handle changes only once nothing can fail any more
      FreshLayout L;
      if (int rc = append_packed_rows(ix, 1, n, nullptr, row_pos.data(), codes, L)) return rc;
      int32_t* new_ids = nullptr;
      if (int rc = grown_copy(ix->ids, (size_t)old_n, (size_t)(old_n + n), ids, (size_t)n, &new_ids)) return grow_failed(rc);
      ix->h_ids.reserve(ix->h_ids.size() + (size_t)n);   // (may throw: before anything has changed)
      install_layout(ix, L);
      swap_grown(&ix->ids, (size_t)old_n, (size_t)(old_n + n), new_ids, &ix->bytes);
      ix->h_ids.insert(ix->h_ids.end(), ids, ids + n);
      ix->max_id = ids[n - 1];
      if (ix->pq_shadow) { free_index(ix->pq_shadow); ix->pq_shadow = nullptr; }   // (rebuilt by the next batch search)
      return FREDDY_OK;
    }
    case KIND_IVF: {
      if (!codes || !coarse_id) return fail(FREDDY_E_ARG, "coarse_id and codes are required");
      FreshLayout L;   // (the block layout, the one-byte codes and the row terms: all beside the pinned ones)
      if (int rc = append_packed_rows(ix, ix->C, n, coarse_id, ids, codes, L)) return rc;
      install_layout(ix, L);
      ix->max_id = ids[n - 1];
      return FREDDY_OK;
    }
    case KIND_IVPQ: {
      JoinIndex& j = ix->join;
      if (!codes || !coarse_id || (j.has_vectors && !vectors)) return fail(FREDDY_E_ARG, "coarse_id, codes (and vectors, if pinned) are required");
      for (int64_t i = 0; i < n; ++i) {
        if (coarse_id[i] < 0 || coarse_id[i] >= j.cells) return fail(FREDDY_E_ARG, "coarse_id %d out of range", coarse_id[i]);
        for (int l = 0; l < j.m; ++l)
          if (codes[(size_t)i * j.m + l] < 0 || codes[(size_t)i * j.m + l] >= j.K) return fail(FREDDY_E_ARG, "code out of range at new row %lld", (long long)i);
      }
      const size_t o = (size_t)j.N, nn = (size_t)(j.N + n);
      // every longer array and the longer scratch bitmap beside the pinned ones; the handle changes only once all of them exist
      int32_t *new_ids = nullptr, *new_cell = nullptr;
      int16_t* new_codes = nullptr;
      float* new_vec = nullptr;
      uint32_t* new_mark = nullptr;
      int rc = grown_copy(j.ids, o, nn, ids, (size_t)n, &new_ids);
      if (!rc) rc = grown_copy(j.cell, o, nn, coarse_id, (size_t)n, &new_cell);
      if (!rc) rc = grown_copy(j.codes, o * j.MP, nn * j.MP, join_pad_codes(codes, n, j.m, j.MP).data(), (size_t)n * j.MP, &new_codes);
      if (!rc && j.has_vectors) rc = grown_copy(j.vectors, o * j.d, nn * j.d, vectors, (size_t)n * j.d, &new_vec);
      if (!rc && dev_malloc(&new_mark, sizeof(uint32_t) * ((nn + 31) / 32 + 1)) != hipSuccess) { new_mark = nullptr; rc = -1; }
      if (rc) {
        void* fresh[] = {new_ids, new_cell, new_codes, new_vec, new_mark};
        for (void* p : fresh) if (p) (void)dev_free(p);
        return grow_failed(rc);
      }
      j.h_ids.reserve(j.h_ids.size() + (size_t)n); j.h_cell.reserve(j.h_cell.size() + (size_t)n);
      swap_grown(&j.ids, o, nn, new_ids, &ix->bytes);
      swap_grown(&j.cell, o, nn, new_cell, &ix->bytes);
      swap_grown(&j.codes, o * j.MP, nn * j.MP, new_codes, &ix->bytes);
      if (j.has_vectors) swap_grown(&j.vectors, o * j.d, nn * j.d, new_vec, &ix->bytes);
      if (j.markbits) (void)dev_free(j.markbits);
      j.markbits = new_mark;
      j.h_ids.insert(j.h_ids.end(), ids, ids + n);
      j.h_cell.insert(j.h_cell.end(), coarse_id, coarse_id + n);
      j.N += n; ix->N = j.N;
      j.ids_affine = (int64_t)j.h_ids.back() - j.h_ids.front() == j.N - 1;
      return FREDDY_OK;
    }
    case KIND_VEC: {
      if (!vectors) return fail(FREDDY_E_ARG, "vectors are required");
      const int d = ix->d;
      const size_t o = (size_t)ix->N, nn = (size_t)(ix->N + n);
      const int64_t new_blocks = (int64_t)((nn + 63) / 64);
      // the longer blocked copy, row-major copy and ids beside the pinned ones; the handle changes only once all three are complete
      float *xb = nullptr, *new_rows = nullptr;
      int32_t* new_ids = nullptr;
      int rc = 0;
      if (dev_malloc(&xb, sizeof(float) * (size_t)new_blocks * d * 64) != hipSuccess) { xb = nullptr; rc = fail(FREDDY_E_NOMEM, "device allocation failed while appending rows"); }
      if (!rc && (hipMemset(xb, 0, sizeof(float) * (size_t)new_blocks * d * 64) != hipSuccess ||
                  (ix->n_blocks && hipMemcpy(xb, ix->xb, sizeof(float) * (size_t)ix->n_blocks * d * 64, hipMemcpyDeviceToDevice) != hipSuccess)))
        rc = fail(FREDDY_E_HIP, "copying the row blocks failed");
      if (!rc) { if (const int g = grown_copy(ix->coarse, o * d, nn * d, vectors, (size_t)n * d, &new_rows)) rc = grow_failed(g); }
      if (!rc) { if (const int g = grown_copy(ix->ids, o, nn, ids, (size_t)n, &new_ids)) rc = grow_failed(g); }
      if (!rc) {
        hipLaunchKernelGGL(place_vectors_kernel, dim3((unsigned)n), dim3(256), 0, ix->stream, new_rows + o * d, (int64_t)o, n, xb, d);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "re-blocking the new rows failed");
      }
      if (rc) {
        void* fresh[] = {xb, new_rows, new_ids};
        for (void* p : fresh) if (p) (void)dev_free(p);
        return rc;
      }
      ix->h_ids.reserve(ix->h_ids.size() + (size_t)n);
      swap_grown(&ix->coarse, o * d, nn * d, new_rows, &ix->bytes);
      swap_grown(&ix->ids, o, nn, new_ids, &ix->bytes);
      if (ix->xb) (void)dev_free(ix->xb);
      ix->bytes += (int64_t)sizeof(float) * d * 64 * (new_blocks - std::max<int64_t>(ix->n_blocks, 1));   // (pin_vectors counts one block at least)
      ix->xb = xb; ix->n_blocks = new_blocks; ix->N += n;
      ix->h_ids.insert(ix->h_ids.end(), ids, ids + n);
      // the filter's scale and norm bound cover the new rows.  The statistics and the fragment copy are rewritten in place: a
      // failure from here on leaves rows the filter's state does not cover -> the handle is poisoned
      if (int rc2 = exf_table_stats(ix, (int64_t)o, n)) { ix->poisoned = true; return rc2; }
      return FREDDY_OK;
    }
  }
  return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
}

// ---------------------------------------------------------------------------------------
// remove_rows: the DELETE beside insert_batch's INSERTs (kernels in remove_kernels.h)
// ---------------------------------------------------------------------------------------
// device scratch of one call, freed when it goes out of scope
struct RemoveScratch {
  std::vector<void*> held;
  ~RemoveScratch() { for (void* p : held) if (p) (void)dev_free(p); }
  template <class T> T* get(size_t n) {
    void* p = nullptr;
    if (dev_malloc(&p, sizeof(T) * std::max<size_t>(n, 1)) != hipSuccess) return nullptr;
    held.push_back(p);
    return static_cast<T*>(p);
  }
  template <class T> T* put(const T* src, size_t n) {
    T* p = get<T>(n);
    if (p && n && hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
  }
};

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

// A fresh device array of the rows that stay (max(n_new * e, 1) elements, as upload() sizes it), enqueued on `s`: *out is the
// caller's to swap in or free.  A row is e elements of T, a whole number of 4-byte words.
template <class T>
static int gather_rows(hipStream_t s, const T* src, int64_t n_new, int e, const int32_t* d_rm, int n_rm, T** out) {
  *out = nullptr;
  if (dev_malloc((void**)out, sizeof(T) * std::max<size_t>((size_t)n_new * e, 1)) != hipSuccess) { *out = nullptr; return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows"); }
  if (n_new > 0) {
    hipLaunchKernelGGL(rm_gather_rows_kernel, dim3((unsigned)((n_new + 63) / 64)), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(src),
                       reinterpret_cast<uint32_t*>(*out), d_rm, n_rm, n_new, (int)(sizeof(T) * e / 4));
    HIP_TRY(hipGetLastError());
  }
  return 0;
}
// what `bytes` gains when an array that upload() counted goes from old_n to new_n elements
template <class T>
static int64_t resized_bytes(size_t old_n, size_t new_n) { return (int64_t)sizeof(T) * ((int64_t)std::max<size_t>(new_n, 1) - (int64_t)std::max<size_t>(old_n, 1)); }

// rows of a pq / ivf index: every slot whose pos is in `rm` (ascending, distinct: ids of an ivf handle, row indices of the flat
// table) leaves; the rows that stay keep their order inside their list.  The new block layout is built beside the old one on
// the device and swapped in; nothing changes when no slot matches.  *removed: the rows that left; *max_pos: the largest pos
// that stays (-1: none).  The lists lose part of arrange_list_rows' bank-conflict arrangement (speed only).
// Everything is built into L: the handle is not touched, and L.ready stays false when there is nothing to change.
static int remove_packed_rows(freddy_gpu_index* ix, int n_lists, const std::vector<int32_t>& rm, bool renumber, int64_t* removed, int32_t* max_pos, FreshLayout& L) {
  const int M2 = ix->M2;
  const int64_t ob = ix->n_blocks;
  *removed = 0;
  if (ob <= 0 || rm.empty()) return 0;
  RemoveScratch tmp;
  const int32_t minus_one = -1;
  int32_t* d_rm = tmp.put(rm.data(), rm.size());
  unsigned long long* keep_mask = tmp.get<unsigned long long>((size_t)ob);
  int32_t *keep_cnt = tmp.get<int32_t>((size_t)ob), *prefix = tmp.get<int32_t>((size_t)ob), *list_keep = tmp.get<int32_t>((size_t)n_lists);
  int32_t* d_max = tmp.put(&minus_one, 1);
  if (!d_rm || !keep_mask || !keep_cnt || !prefix || !list_keep || !d_max) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  hipLaunchKernelGGL(rm_mark_kernel, dim3((unsigned)((ob + 3) / 4)), dim3(256), 0, ix->stream, ix->pos, ob, d_rm, (int)rm.size(), keep_mask, keep_cnt, d_max);
  hipLaunchKernelGGL(rm_list_scan_kernel, dim3((unsigned)n_lists), dim3(256), 0, ix->stream, ix->blk_off, keep_cnt, prefix, list_keep);
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> keep((size_t)n_lists);
  HIP_TRY(hipMemcpyAsync(keep.data(), list_keep, sizeof(int32_t) * (size_t)n_lists, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipMemcpyAsync(max_pos, d_max, sizeof(int32_t), hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  std::vector<int32_t> new_list_off((size_t)n_lists + 1, 0), new_blk((size_t)n_lists + 1, 0);
  int max_blocks = 0;
  for (int c = 0; c < n_lists; ++c) {
    if (keep[(size_t)c] < 0 || keep[(size_t)c] > ix->h_list_off[(size_t)c + 1] - ix->h_list_off[(size_t)c])
      return fail(FREDDY_E_HIP, "list %d keeps %d of its %d rows: the pinned layout is inconsistent", c, keep[(size_t)c], ix->h_list_off[(size_t)c + 1] - ix->h_list_off[(size_t)c]);
    new_list_off[(size_t)c + 1] = new_list_off[(size_t)c] + keep[(size_t)c];
    const int nb = (keep[(size_t)c] + 63) / 64;
    new_blk[(size_t)c + 1] = new_blk[(size_t)c] + nb;
    max_blocks = std::max(max_blocks, nb);
  }
  const int64_t kept = new_list_off[(size_t)n_lists];
  if (kept == ix->N) return 0;   // (no pinned row has one of the ids)
  const int64_t nnb = new_blk[(size_t)n_lists], alloc_blocks = std::max<int64_t>(nnb, 1);
  std::vector<int32_t> blk_cell((size_t)alloc_blocks, 0);
  for (int c = 0; c < n_lists; ++c)
    for (int b = new_blk[(size_t)c]; b < new_blk[(size_t)c + 1]; ++b) blk_cell[(size_t)b] = c;
  uint32_t* packed = nullptr;
  int32_t *pos = nullptr, *d_blk_cell = nullptr, *d_new_blk = nullptr, *d_list_off = nullptr;
  int64_t junk = 0;
  int rc = 0;
  if (dev_malloc((void**)&packed, sizeof(uint32_t) * (size_t)alloc_blocks * M2 * 64) != hipSuccess ||
      dev_malloc((void**)&pos, sizeof(int32_t) * (size_t)alloc_blocks * 64) != hipSuccess ||
      upload(&d_blk_cell, blk_cell.data(), blk_cell.size(), &junk) || upload(&d_new_blk, new_blk.data(), new_blk.size(), &junk) ||
      upload(&d_list_off, new_list_off.data(), new_list_off.size(), &junk))
    rc = fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  if (!rc && nnb == 0 &&   // (an empty table keeps one block of padding, as pack_lists leaves it)
      (hipMemsetAsync(packed, 0, sizeof(uint32_t) * (size_t)M2 * 64, ix->stream) != hipSuccess || hipMemsetAsync(pos, 0xff, sizeof(int32_t) * 64, ix->stream) != hipSuccess))
    rc = fail(FREDDY_E_HIP, "clearing the empty table failed");
  if (!rc && nnb > 0) {
    hipLaunchKernelGGL(rm_scatter_kernel, dim3((unsigned)((ob + 3) / 4)), dim3(256), 0, ix->stream, ix->packed, ix->pos, ix->blk_cell, d_new_blk, keep_mask,
                       prefix, ob, nnb * 64, M2, renumber ? 1 : 0, packed, pos);
    hipLaunchKernelGGL(rm_fill_tail_kernel, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0, ix->stream, d_list_off, d_new_blk, n_lists, M2, packed, pos);
  }
  if (!rc && (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess)) rc = fail(FREDDY_E_HIP, "compacting the lists failed");
  L.packed = packed; L.pos = pos; L.blk_cell = d_blk_cell; L.blk_off = d_new_blk; L.list_off = d_list_off;   // (L frees them if it is never installed)
  if (rc) { L.drop(); return rc; }
  L.n_blocks = nnb;
  L.max_list_blocks = max_blocks;
  L.h_list_off = new_list_off;
  L.N = kept;
  if (int rc2 = finish_layout(ix, L)) return rc2;
  *removed = ix->N - kept;
  return 0;
}

extern "C" int freddy_gpu_remove_rows(freddy_gpu_index_t* ix, int64_t n, const int32_t* ids, int64_t* removed) {
  if (n < 0 || (n > 0 && !ids)) return fail(FREDDY_E_ARG, "bad argument: n = %lld ids%s", (long long)n, ids ? "" : ", no ids");
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (removed) *removed = 0;
  if (n == 0) return FREDDY_OK;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0) return fail(FREDDY_E_ARG, "id %d at position %lld is negative (-1 is the filler of a result list)", ids[i], (long long)i);
  if (!ix->replicas.empty()) {   // the rule of append_rows: the primary first, a failure after the first device has changed poisons the handle
    std::vector<freddy_gpu_index*> reps;
    reps.swap(ix->replicas);
    int rc = freddy_gpu_remove_rows(ix, n, ids, removed);
    reps.swap(ix->replicas);
    if (rc) return rc;   // (the primary is as it was, or has poisoned itself: no other device has changed)
    for (freddy_gpu_index* r : ix->replicas)
      if ((rc = freddy_gpu_remove_rows(r, n, ids, nullptr))) { ix->poisoned = true; return rc; }
    return FREDDY_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  std::vector<int32_t> want(ids, ids + n);   // any order, an id listed twice counts once
  std::sort(want.begin(), want.end());
  want.erase(std::unique(want.begin(), want.end()), want.end());
  int64_t gone = 0;
  switch (ix->kind) {
    case KIND_PQ: {
      const std::vector<int32_t> rows = rows_of_ids(ix->h_ids, want.data(), (int64_t)want.size());   // flat table: pos = row index
      if (rows.empty()) return FREDDY_OK;
      const int64_t old_n = ix->N, new_n = old_n - (int64_t)rows.size();
      RemoveScratch tmp;
      int32_t* d_rm = tmp.put(rows.data(), rows.size());
      if (!d_rm) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
      int32_t* new_ids = nullptr;
      if (int rc = gather_rows(ix->stream, ix->ids, new_n, 1, d_rm, (int)rows.size(), &new_ids)) {
        (void)hipStreamSynchronize(ix->stream);   // (the gather may be in flight: it has left new_ids before the array goes back)
        if (new_ids) (void)dev_free(new_ids);
        return rc;
      }
      int32_t unused = -1;
      FreshLayout L;
      if (int rc = remove_packed_rows(ix, 1, rows, true, &gone, &unused, L)) {   // (synchronises the stream: new_ids is complete)
        (void)hipStreamSynchronize(ix->stream);
        (void)dev_free(new_ids);
        return rc;
      }
      if (!L.ready) { (void)hipStreamSynchronize(ix->stream); (void)dev_free(new_ids); return fail(FREDDY_E_HIP, "rows %d.. have no slot: the pinned layout is inconsistent", rows[0]); }
      install_layout(ix, L);
      // views of the flat table are rebuilt from the new layout on next use
      if (ix->pq_shadow) { free_index(ix->pq_shadow); ix->pq_shadow = nullptr; }
      if (ix->pq_sub_view) { free_index(ix->pq_sub_view); ix->pq_sub_view = nullptr; }
      if (ix->ids) (void)dev_free(ix->ids);
      ix->ids = new_ids;
      ix->bytes += resized_bytes<int32_t>((size_t)old_n, (size_t)new_n);
      erase_rows(ix->h_ids, rows);
      ix->max_id = ix->h_ids.empty() ? -1 : ix->h_ids.back();
      break;
    }
    case KIND_IVF: {
      int32_t max_pos = -1;
      FreshLayout L;   // (the compacted lists, their one-byte codes and row terms: all beside the pinned ones)
      if (int rc = remove_packed_rows(ix, ix->C, want, false, &gone, &max_pos, L)) return rc;   // (pos holds the ids)
      if (L.ready) {
        install_layout(ix, L);
        ix->max_id = max_pos;   // a later append may start above the largest id that is left, as on a fresh pin
      }
      break;
    }
    case KIND_IVPQ: {
      JoinIndex& j = ix->join;
      const std::vector<int32_t> rows = rows_of_ids(j.h_ids, want.data(), (int64_t)want.size());
      if (rows.empty()) return FREDDY_OK;
      const size_t o = (size_t)j.N, nn = o - rows.size();
      RemoveScratch tmp;
      int32_t* d_rm = tmp.put(rows.data(), rows.size());
      uint32_t* markbits = tmp.get<uint32_t>((nn + 31) / 32 + 1);
      if (!d_rm || !markbits) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
      int32_t *new_ids = nullptr, *new_cell = nullptr;
      int16_t* new_codes = nullptr;
      float* new_vec = nullptr;
      int rc = gather_rows(ix->stream, j.ids, (int64_t)nn, 1, d_rm, (int)rows.size(), &new_ids);
      if (!rc) rc = gather_rows(ix->stream, j.cell, (int64_t)nn, 1, d_rm, (int)rows.size(), &new_cell);
      if (!rc) rc = gather_rows(ix->stream, j.codes, (int64_t)nn, j.MP, d_rm, (int)rows.size(), &new_codes);
      if (!rc && j.has_vectors) rc = gather_rows(ix->stream, j.vectors, (int64_t)nn, j.d, d_rm, (int)rows.size(), &new_vec);
      if (!rc && hipStreamSynchronize(ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "compacting the ivpq rows failed");
      if (rc) {
        void* fresh[] = {new_ids, new_cell, new_codes, new_vec};
        for (void* p : fresh) if (p) (void)dev_free(p);
        return rc;
      }
      void* old[] = {j.ids, j.cell, j.codes, j.vectors, j.markbits};
      for (void* p : old) if (p) (void)dev_free(p);
      j.ids = new_ids; j.cell = new_cell; j.codes = new_codes; j.vectors = new_vec;
      j.markbits = markbits; tmp.held.erase(std::find(tmp.held.begin(), tmp.held.end(), (void*)markbits));
      ix->bytes += 2 * resized_bytes<int32_t>(o, nn) + resized_bytes<int16_t>(o * j.MP, nn * j.MP) + (j.has_vectors ? resized_bytes<float>(o * j.d, nn * j.d) : 0);
      erase_rows(j.h_ids, rows);
      erase_rows(j.h_cell, rows);
      j.N = (int64_t)nn; ix->N = j.N;
      j.ids_affine = j.N > 0 && (int64_t)j.h_ids.back() - j.h_ids.front() == j.N - 1;   // (a hole in the middle: binary search from now on)
      j.tl_valid = false;   // (the cached "id IN (targets)" resolution refers to the rows as they were)
      gone = (int64_t)rows.size();
      break;
    }
    case KIND_VEC: {
      const std::vector<int32_t> rows = rows_of_ids(ix->h_ids, want.data(), (int64_t)want.size());
      if (rows.empty()) return FREDDY_OK;
      const int d = ix->d;
      const size_t o = (size_t)ix->N, nn = o - rows.size();
      const int64_t new_blocks = (int64_t)((nn + 63) / 64), alloc_blocks = std::max<int64_t>(new_blocks, 1);
      const int64_t same_blocks = std::min<int64_t>(rows[0] / 64, new_blocks);   // (the blocks before the first row that leaves stay as they are)
      const size_t blk = sizeof(float) * (size_t)d * 64;
      RemoveScratch tmp;
      int32_t* d_rm = tmp.put(rows.data(), rows.size());
      if (!d_rm) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
      int32_t* new_ids = nullptr;
      float *new_rows = nullptr, *xb = nullptr;
      int rc = gather_rows(ix->stream, ix->ids, (int64_t)nn, 1, d_rm, (int)rows.size(), &new_ids);
      if (!rc) rc = gather_rows(ix->stream, ix->coarse, (int64_t)nn, d, d_rm, (int)rows.size(), &new_rows);
      if (!rc && dev_malloc((void**)&xb, blk * (size_t)alloc_blocks) != hipSuccess) { xb = nullptr; rc = fail(FREDDY_E_NOMEM, "device allocation failed while removing rows"); }
      if (!rc && same_blocks > 0 && hipMemcpyAsync(xb, ix->xb, blk * (size_t)same_blocks, hipMemcpyDeviceToDevice, ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "copying the row blocks failed");
      if (!rc && alloc_blocks > same_blocks && hipMemsetAsync(xb + (size_t)same_blocks * d * 64, 0, blk * (size_t)(alloc_blocks - same_blocks), ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "clearing the row blocks failed");
      if (!rc && (int64_t)nn > same_blocks * 64) {
        const int64_t first = same_blocks * 64, cnt = (int64_t)nn - first;
        hipLaunchKernelGGL(place_vectors_kernel, dim3((unsigned)cnt), dim3(256), 0, ix->stream, new_rows + (size_t)first * d, first, cnt, xb, d);
        if (hipGetLastError() != hipSuccess) rc = fail(FREDDY_E_HIP, "re-blocking the rows failed");
      }
      if (!rc && hipStreamSynchronize(ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "compacting the vector rows failed");
      if (rc) {
        void* fresh[] = {new_ids, new_rows, xb};
        for (void* p : fresh) if (p) (void)dev_free(p);
        return rc;
      }
      void* old[] = {ix->ids, ix->coarse, ix->xb};
      for (void* p : old) if (p) (void)dev_free(p);
      ix->bytes += resized_bytes<int32_t>(o, nn) + (int64_t)blk * (alloc_blocks - std::max<int64_t>(ix->n_blocks, 1));
      if (nn == 0) {   // (pin_vectors keeps no row-major copy of an empty table)
        (void)dev_free(new_rows); new_rows = nullptr;
        ix->bytes -= (int64_t)sizeof(float) * (int64_t)o * d;
      } else ix->bytes += (int64_t)sizeof(float) * d * ((int64_t)nn - (int64_t)o);
      ix->ids = new_ids; ix->coarse = new_rows; ix->xb = xb;
      ix->n_blocks = new_blocks; ix->N = (int64_t)nn;
      erase_rows(ix->h_ids, rows);
      gone = (int64_t)rows.size();
      // the exact filter's state over the rows that are left, as a fresh pin computes it: a larger scale once the row with the
      // largest element has gone, the filter back on once the only non-finite row has (the fragment copy keeps its capacity)
      if (nn == 0) ix->exf_ok = false;
      else if (int rc2 = exf_table_stats(ix, 0, (int64_t)nn)) { ix->poisoned = true; return rc2; }   // (the statistics are rewritten in place: the rows have gone, the filter's state has not followed)
      break;
    }
    default: return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  }
  if (removed) *removed = gone;
  return FREDDY_OK;
}

// ---------------------------------------------------------------------------------------
// update_rows: the UPDATE of a row -- the id stays, the payload changes (kernels in update_kernels.h)
// ---------------------------------------------------------------------------------------
// The slots (block * 64 + lane) and lists of the rows whose pos is one of `upd` (ascending, distinct), -1 where no slot has it.
// Synchronises the stream.  Every pair is checked against the layout before the caller hands it to a kernel.
static int locate_packed_rows(freddy_gpu_index* ix, int n_lists, const std::vector<int32_t>& upd, std::vector<int64_t>& slot, std::vector<int32_t>& cell) {
  const size_t n = upd.size();
  slot.assign(n, -1);
  cell.assign(n, 0);
  if (ix->n_blocks <= 0 || n == 0) return 0;
  RemoveScratch tmp;
  int32_t* d_upd = tmp.put(upd.data(), n);
  int64_t* d_slot = tmp.get<int64_t>(n);
  int32_t* d_cell = tmp.get<int32_t>(n);
  if (!d_upd || !d_slot || !d_cell) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
  HIP_TRY(hipMemsetAsync(d_slot, 0xff, sizeof(int64_t) * n, ix->stream));
  HIP_TRY(hipMemsetAsync(d_cell, 0, sizeof(int32_t) * n, ix->stream));
  hipLaunchKernelGGL(up_locate_kernel, dim3((unsigned)((ix->n_blocks + 3) / 4)), dim3(256), 0, ix->stream, ix->pos, ix->blk_cell, ix->n_blocks, d_upd, (int)n,
                     d_slot, d_cell);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(slot.data(), d_slot, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipMemcpyAsync(cell.data(), d_cell, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  for (size_t j = 0; j < n; ++j)
    if (slot[j] < -1 || slot[j] >= ix->n_blocks * 64 || (slot[j] >= 0 && (cell[j] < 0 || cell[j] >= n_lists)))
      return fail(FREDDY_E_HIP, "row %d sits in slot %lld of list %d: the pinned layout is inconsistent", upd[j], (long long)slot[j], cell[j]);
  return 0;
}

// the code words of n rows rewritten in their slots (pos keeps its value: row_pos[i] is what the slot holds already)
static int rewrite_packed_rows(freddy_gpu_index* ix, const std::vector<int64_t>& slot, const std::vector<int32_t>& row_pos, const std::vector<int16_t>& codes) {
  const size_t n = slot.size();
  if (n == 0) return 0;
  RemoveScratch tmp;
  int64_t* d_slot = tmp.put(slot.data(), n);
  int32_t* d_pos = tmp.put(row_pos.data(), n);
  int16_t* d_codes = tmp.put(codes.data(), codes.size());
  if (!d_slot || !d_pos || !d_codes) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
  hipLaunchKernelGGL(place_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, d_slot, d_pos, d_codes, (int64_t)n, ix->packed, ix->pos, ix->m, ix->M2);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) return fail(FREDDY_E_HIP, "rewriting the rows' codes failed");
  return 0;
}

// dst row rows[j] <- the j-th of n host rows of e elements of T (a whole number of 4-byte words), enqueued on the stream
template <class T>
static int scatter_rows(freddy_gpu_index* ix, RemoveScratch& tmp, const T* h_src, int64_t n, int e, const int32_t* d_rows, T* dst) {
  T* d_src = tmp.put(h_src, (size_t)n * e);
  if (!d_src) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
  const int wpr = (int)(sizeof(T) * e / 4);
  hipLaunchKernelGGL(up_scatter_rows_kernel, dim3((unsigned)((n * wpr + 255) / 256)), dim3(256), 0, ix->stream, reinterpret_cast<const uint32_t*>(d_src),
                     reinterpret_cast<uint32_t*>(dst), d_rows, n, wpr);
  HIP_TRY(hipGetLastError());
  return 0;
}

// What the call does once its arguments have passed: known[] = positions (in the caller's arrays) of the ids a pinned row has,
// rows[] = their row indices (flat kinds) -- both in ascending row order.  Arrays are written in place.
static int update_rows_checked(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, const float* vectors,
                               int64_t* changed, bool* wrote) {
  *changed = 0;
  *wrote = false;
  auto flat_rows = [&](const std::vector<int32_t>& h_ids, std::vector<int32_t>& rows, std::vector<int64_t>& known) {
    std::vector<std::pair<int32_t, int64_t>> hit;
    for (int64_t i = 0; i < n; ++i)
      if (const int32_t r = row_of(h_ids, ids[i]); r >= 0) hit.emplace_back(r, i);
    std::sort(hit.begin(), hit.end());
    for (auto& h : hit) { rows.push_back(h.first); known.push_back(h.second); }
  };
  switch (ix->kind) {
    case KIND_PQ: {
      std::vector<int32_t> rows, cell;
      std::vector<int64_t> known, slot;
      flat_rows(ix->h_ids, rows, known);
      if (rows.empty()) return 0;
      if (int rc = locate_packed_rows(ix, 1, rows, slot, cell)) return rc;   // flat table: pos = row index
      std::vector<int16_t> new_codes(rows.size() * (size_t)ix->m);
      for (size_t j = 0; j < rows.size(); ++j) {
        if (slot[j] < 0) return fail(FREDDY_E_HIP, "row %d has no slot: the pinned layout is inconsistent", rows[j]);
        std::copy(codes + (size_t)known[j] * ix->m, codes + (size_t)(known[j] + 1) * ix->m, new_codes.begin() + j * (size_t)ix->m);
      }
      // views of the flat table are rebuilt from the new codes on next use
      if (ix->pq_shadow) { free_index(ix->pq_shadow); ix->pq_shadow = nullptr; }
      if (ix->pq_sub_view) { free_index(ix->pq_sub_view); ix->pq_sub_view = nullptr; }
      *wrote = true;
      if (int rc = rewrite_packed_rows(ix, slot, rows, new_codes)) return rc;
      *changed = (int64_t)rows.size();
      return build_packed8(ix);
    }
    case KIND_IVF: {
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
        FreshLayout out, in;
        if (int rc = remove_packed_rows(ix, ix->C, move_id, false, &gone, &unused, out)) return rc;
        if (out.ready) install_layout(ix, out);
        *changed += gone;
        if (gone != (int64_t)move_id.size()) return fail(FREDDY_E_HIP, "%lld of %zu rows left their lists: the pinned layout is inconsistent", (long long)gone, move_id.size());
        if (int rc = append_packed_rows(ix, ix->C, (int64_t)move_id.size(), move_cell.data(), move_id.data(), move_codes.data(), in)) return rc;
        install_layout(ix, in);   // (with the one-byte codes and the row terms of the final layout)
        ix->max_id = max_id;      // no id has come or gone
        return 0;
      }
      if (int rc = build_packed8(ix)) return rc;
      ix->max_id = max_id;
      return refresh_row_terms(ix);
    }
    case KIND_IVPQ: {
      JoinIndex& j = ix->join;
      std::vector<int32_t> rows;
      std::vector<int64_t> known;
      flat_rows(j.h_ids, rows, known);
      if (rows.empty()) return 0;
      const size_t k = rows.size();
      std::vector<int32_t> new_cell(k);
      std::vector<int16_t> new_codes(k * (size_t)j.m);
      std::vector<float> new_vec(j.has_vectors ? k * (size_t)j.d : 0);
      for (size_t r = 0; r < k; ++r) {
        new_cell[r] = coarse_id[known[r]];
        std::copy(codes + (size_t)known[r] * j.m, codes + (size_t)(known[r] + 1) * j.m, new_codes.begin() + r * (size_t)j.m);
        if (j.has_vectors) std::copy(vectors + (size_t)known[r] * j.d, vectors + (size_t)(known[r] + 1) * j.d, new_vec.begin() + r * (size_t)j.d);
      }
      RemoveScratch tmp;
      int32_t* d_rows = tmp.put(rows.data(), k);
      if (!d_rows) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
      j.tl_valid = false;   // (the cached target lists are bucketed by cell)
      *wrote = true;
      int rc = scatter_rows(ix, tmp, new_cell.data(), (int64_t)k, 1, d_rows, j.cell);
      if (!rc) rc = scatter_rows(ix, tmp, join_pad_codes(new_codes.data(), (int64_t)k, j.m, j.MP).data(), (int64_t)k, j.MP, d_rows, j.codes);
      if (!rc && j.has_vectors) rc = scatter_rows(ix, tmp, new_vec.data(), (int64_t)k, j.d, d_rows, j.vectors);
      if (!rc) *changed = (int64_t)k;
      if (hipStreamSynchronize(ix->stream) != hipSuccess && !rc) rc = fail(FREDDY_E_HIP, "rewriting the ivpq rows failed");
      if (rc) return rc;
      for (size_t r = 0; r < k; ++r) j.h_cell[(size_t)rows[r]] = new_cell[r];
      return 0;
    }
    case KIND_VEC: {
      std::vector<int32_t> rows;
      std::vector<int64_t> known;
      flat_rows(ix->h_ids, rows, known);
      if (rows.empty()) return 0;
      const size_t k = rows.size();
      const int d = ix->d;
      std::vector<float> new_vec(k * (size_t)d);
      for (size_t r = 0; r < k; ++r) std::copy(vectors + (size_t)known[r] * d, vectors + (size_t)(known[r] + 1) * d, new_vec.begin() + r * (size_t)d);
      {
        RemoveScratch tmp;
        int32_t* d_rows = tmp.put(rows.data(), k);
        float* d_src = tmp.put(new_vec.data(), new_vec.size());
        if (!d_rows || !d_src) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
        *wrote = true;
        hipLaunchKernelGGL(up_scatter_rows_kernel, dim3((unsigned)(((int64_t)k * d + 255) / 256)), dim3(256), 0, ix->stream, reinterpret_cast<const uint32_t*>(d_src),
                           reinterpret_cast<uint32_t*>(ix->coarse), d_rows, (int64_t)k, d);
        hipLaunchKernelGGL(up_place_vectors_kernel, dim3((unsigned)k), dim3(256), 0, ix->stream, d_src, d_rows, (int64_t)k, ix->xb, d);
        *changed = (int64_t)k;
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) return fail(FREDDY_E_HIP, "rewriting the vector rows failed");
      }
      // the exact filter's state over all rows, as a fresh pin computes it (the old values have left the statistics); the fragment
      // copy: the strips of the updated rows, or every strip when the scale moved or the filter came back
      std::vector<int32_t> strips;
      for (int32_t r : rows)
        if (strips.empty() || strips.back() != r / 32) strips.push_back(r / 32);
      return exf_table_stats(ix, 0, ix->N, &strips);
    }
  }
  return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
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
    for (int64_t i = 0; i < n; ++i) {
      if (!flat && (coarse_id[i] < 0 || coarse_id[i] >= cells))
        return fail(FREDDY_E_ARG, "coarse_id %d of update row %lld is outside [0, %d)", coarse_id[i], (long long)i, cells);
      for (int l = 0; l < m; ++l)
        if (codes[(size_t)i * m + l] < 0 || codes[(size_t)i * m + l] >= K)
          return fail(FREDDY_E_ARG, "code %d of update row %lld position %d is outside [0, %d)", (int)codes[(size_t)i * m + l], (long long)i, l, K);
    }
  }
  if (!ix->replicas.empty()) {   // the rule of append_rows: the primary first, a failure after the first device has changed poisons the handle
    std::vector<freddy_gpu_index*> reps;
    reps.swap(ix->replicas);
    int64_t changed = 0;
    int rc = freddy_gpu_update_rows(ix, n, ids, coarse_id, codes, vectors, &changed);
    reps.swap(ix->replicas);
    if (rc) return rc;          // (the primary has poisoned itself if it had written anything)
    for (freddy_gpu_index* r : ix->replicas)
      if ((rc = freddy_gpu_update_rows(r, n, ids, coarse_id, codes, vectors, nullptr))) { ix->poisoned = true; return rc; }
    if (updated) *updated = changed;   // (only once every replica has followed)
    return FREDDY_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  int64_t changed = 0;
  bool wrote = false;
  const int rc = update_rows_checked(ix, n, ids, coarse_id, codes, vectors, &changed, &wrote);
  if (rc) {
    if (wrote) ix->poisoned = true;   // arrays are written in place: a failure after the first write leaves a table that is neither the old nor the new one
    return rc;
  }
  if (updated) *updated = changed;
  return FREDDY_OK;
}

extern "C" int freddy_gpu_update_codebook(freddy_gpu_index_t* ix, const float* codebook) {
  if (!ix || !codebook) return fail(FREDDY_E_ARG, "NULL argument");
  if (!ix->replicas.empty()) {   // every device or none: a failure after the first device has changed poisons the handle
    size_t done = 0;
    int rc = 0;
    for (freddy_gpu_index* r : ix->replicas) { if ((rc = freddy_gpu_update_codebook(r, codebook))) break; ++done; }
    if (!rc) {
      std::vector<freddy_gpu_index*> none;
      none.swap(ix->replicas);
      rc = freddy_gpu_update_codebook(ix, codebook);
      none.swap(ix->replicas);
      if (!rc) return FREDDY_OK;
      done = ix->replicas.size();
    }
    if (done > 0) ix->poisoned = true;   // (a device that failed is as it was: only a device that HAS changed makes the handle inconsistent)
    return rc;
  }
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipDeviceSynchronize());   // (searches of every stream and lane have drained before the tables change)
  if (ix->kind == KIND_PQ) return derive_codebook_tables(ix, codebook);
  if (ix->kind == KIND_IVF) {
    return derive_codebook_tables(ix, codebook, true);   // (the row terms follow the codebook: built beside the old ones with the new tables)
  }
  if (ix->kind == KIND_IVPQ) {
    JoinIndex& j = ix->join;
    std::vector<float> cbT((size_t)j.m * j.S * j.K);
    for (int p = 0; p < j.m; ++p)
      for (int c = 0; c < j.K; ++c)
        for (int i = 0; i < j.S; ++i) cbT[((size_t)p * j.S + i) * j.K + c] = codebook[((size_t)p * j.K + c) * j.S + i];
    HIP_TRY(hipMemcpy(j.cbT, cbT.data(), sizeof(float) * cbT.size(), hipMemcpyHostToDevice));
    return FREDDY_OK;
  }
  return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
}

