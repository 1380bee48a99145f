// encode_filter.h -- the index build's encoding step for rows of a vector handle as FILTER + REFINE on the matrix cores
// (freddy_gpu_encode_rows; encode_rows.hip launches what is here).
//
// freddy_gpu_encode evaluates squareDistance (index_utils.c:500-508: (x_j - c_j) rounded, squared, added in order j = 0..S-1 from
// +0) for EVERY (row, centroid) pair: assign_coarse_kernel over C centroids of d dimensions, encode_pq_kernel over K codewords of
// S = d / m dimensions per position -- n (C d + m K S) separately rounded sub / mul / add triples, of which only the argmin per
// (row, position) ever matters.  Here, per ITEM = (row, position) -- the coarse search is one more position of C centroids x d:
//
//   a[c] = |x|^2 + |c|^2 - 2 x.c        x.c on f16-SPLIT operands (v_mfma_f32_32x32x16_f16, fp32 accumulate): every fp32 input is
//                                       hi + lo, hi = f16(v), lo = f16(v - hi) after a power-of-two scaling; x.c ~ hi.hi + hi.lo + lo.hi
//
// with a proven bracket |a[c] - D[c]| <= eps(x) around the reference's binary32 distance D[c].  U = min_c (a[c] + eps) is an upper
// bound of the smallest exact distance, so the nearest centroid -- and every centroid that TIES with it -- has a[c] - eps <= U:
//   1. FILTER  (encode_filter_kernel): a for every centroid of the position; the centroids with a - eps <= U are the item's
//              candidates (1 - 3 of them on real tables);
//   2. REFINE  (encode_refine_kernel): the reference's chain for the candidates and for centroid 0, the argmin of
//              make_key(distance, index) as assign_coarse_kernel / encode_pq_kernel take it: the lowest index among equal distances,
//              and centroid 0 when ITS distance is NaN (the search starts there and nothing is < NaN);
//   3. REDO    the items the filter cannot answer go through the all-exact kernels themselves (encode_rows.hip), compacted.
// The approximate value never reaches an output.  With a coarse quantizer the PQ stage works on the residual r_j = x_j - co_j of
// the row's cell (ONE rounded subtraction per element, residual_kernel's value): the filter stages r, the refine recomputes it.
//
// The bracket (u = 2^-24; |.| Euclidean; E = exact real |x - c|^2 <= (|x| + |c|)^2; S dimensions, T = ceil(S / 16) k-steps):
//   reference chain   |D - E| <= ((1+u)^(S+3) - 1) E                                            S <= 64: 0.40e-5   320: 1.93e-5   512: 3.07e-5
//   dropped lo.lo     <= 2^-22 sum|x_j c_j|;  lo rounded to f16 <= 2 * 2^-22 sum|x_j c_j|  (exact2.h, the same operands)
//   MFMA accumulation a product passes <= 16 in-step adds and the 3 T - 1 accumulations behind it, DOUBLED in case the matrix
//                     core truncates: 2 (3 T + 16) u sum|terms|
//                     dot product in all (3 * 2^-22 + 2 (3 T + 16) u) |x||c|, doubled by the factor 2 of -2 x.c, and
//                     |x||c| <= (|x| + |c|)^2 / 4                                               S <= 64: 0.12e-5   320: 0.26e-5   512: 0.37e-5
//   |x|^2, |c|^2      |x|^2: four fp32 fma chains of <= S / 4 + 1 terms, added (<= (S / 4 + 4) u |x|^2); |c|^2: fp64 sum rounded
//                     once (u |c|^2)                                                            S <= 64: 0.13e-5   320: 0.51e-5   512: 0.79e-5
//   final adds        |x|^2 + |c|^2, the fma with -2 x.c, and the a + eps / a - eps of the comparison: 4 u * 2 (|x| + |c|)^2   0.05e-5
//   sum                                                                                         S <= 64: 0.70e-5   320: 2.75e-5   512: 4.28e-5
//   eps(x) = enc_eps_rel(S) (|x| + max_c |c|)^2 + ENC_EPS_ABS,  enc_eps_rel = 2e-5 (S <= 64), 1.2e-4 (S <= 320: coarse.h's COARSE_EPS,
//   whose derivation for coarse_approx16_body this follows), 2e-4 (S <= 512): 2.8x the sum or more.
//   (|x| from the kernel's own |x|^2, raised by 1e-6; max |c| per position from fp64, raised by 1e-6.)
// The residual.  r_j carries one rounding more than x_j, but the reference's chain starts from the SAME rounded r_j (residual_kernel,
// then encode_pq_kernel): the bracket is a statement about the vector the chain is given, so nothing changes -- |x| is |r|, taken
// from the staged r itself.
// Small magnitudes.  Every operation whose result is subnormal is off by <= 2^-149 absolute instead of u relative; there are at most
// 5 S + 3 T + 24 < 3000 of them: < 5e-42; a square that underflows altogether was below 2^-126, S of them below 6.1e-36, and the
// relative terms of a norm that small are smaller still.  ENC_EPS_ABS = 2e-34 (coarse.h's COARSE_EPS_ABS) covers them.  The unscale factor
// 2^-(ex + ec) is NOT allowed to underflow here: a row whose scale exponents leave [-ENC_MAX_EXP, ENC_MAX_EXP] goes to the redo, so
// the term coarse.h carries for a dropped dot product does not arise.
// An item goes to the redo when (and only when)
//   - more than ENC_KEEP = 16 centroids lie inside the bracket of the running minimum at a tile boundary (below),
//   - its |x|^2, its eps or any a is not finite,
//   - its scale exponents leave the range above,
// or when its whole position does (a non-finite centroid: ENC_POS_EXACT).  Which items those are depends on the inputs alone.
//
// Layouts (host: enc_build_image).  A "position" is K centroids of S dimensions; Kpad = K rounded up to 128, Sp = 16 T.
//   img   [position][Kpad / 32][T][hi / lo][64 lanes][8 halves]: lane = centroid r + 32 g of the group of 32, its 8 values =
//         dimensions 16 t + 8 g .. + 7, scaled by 2^ec[position] -- pin.hip's coarseH.  A wave's operand load is one coalesced 1 KB read.
//   cn2   [position][Kpad] |c|^2 (padding: 0, masked by c < K);  cmax [position];  ec [position]
// The filter kernel.  Grid (position, 64-row tile), 256 threads.  The tile's rows (residuals) are split to f16 hi / lo ONCE, into
// LDS in B-fragment order [2 row groups][T][hi / lo][64 lanes] (lane = row r + 32 g); a pass of 4 threads per row in front takes
// |x|^2 and the largest |element| (the scale).  Then the position's centroids stream by in tiles of 128: wave w owns centroids
// [128 i + 32 w, + 32) as the A operand and both row groups as B -- the CENTROIDS are the rows of the 32 x 32 result and the table
// rows its columns, so that a lane holds 16 centroids of ONE table row per accumulator and the minimum over centroids is 15
// in-lane v_min and one cross-half shuffle (with the table rows as result rows it would be five shuffles per register: 160 per
// tile against 12 matrix instructions at S = 25).  ENC_PF k-steps of A operands are in flight per wave; the next tile's first
// ones are requested before the epilogue.  Per tile:
//   a. every wave lowers U[row] (LDS, atomicMin on the bits of max(a_min + eps, 0): a non-negative float orders as its bits);
//   b. barrier; every lane appends its centroids with a - eps <= U[row] to the row's list (LDS, ENC_CAP = 32 slots);
//   c. barrier; a row with more than ENC_KEEP entries is compacted against the U of step b by ONE thread (rare after the first
//      tiles); still more than ENC_KEEP -> redo.  More than ENC_CAP arrivals in one tile means more than ENC_KEEP new centroids
//      inside the bracket at this boundary: the same rule.
// U only falls, every append of a tile sees the tile's own minimum, and the compaction reads the value step b read: the lists are
// the same SETS in every run (their order is not, and the refine does not depend on it).
// At the end the list is filtered against the final U and written as (count, indices, a), with eps beside it.
// The refine kernel: ONE LANE PER ITEM.  At 1 - 3 candidates per item a wave per item would idle 60 lanes in the subtract / square
// part and the add chain is sequential in j whatever the split; lanes per candidate would need a compaction of (item, candidate)
// pairs in front.  Items are ordered row-major ([row][position]), so the 64 lanes of a wave read 64 consecutive sub-vectors: whole
// cache lines.  Centroid 0 is always evaluated.  The lane counts the candidates, the brackets checked and the brackets violated.
// Option encode_refine_all: the filter also writes every a ([item][Kpad]) and the refine walks all K centroids.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_topk.h"

namespace freddy {

static constexpr int ENC_TQ = 64;          // table rows per workgroup (two 32-column MFMA tiles)
static constexpr int ENC_KEEP = 16;        // candidates an item may have at a tile boundary
static constexpr int ENC_CAP = 32;         // list slots per row in LDS (ENC_KEEP + the arrivals of one tile before the compaction)
static constexpr int ENC_PF = 4;           // k-steps of centroid operands in flight per wave (8 x 1 KB)
static constexpr int ENC_MAX_S = 512;      // the widest search the bracket covers
static constexpr int ENC_MAX_EXP = 120;    // |scale exponent| of a row, of a position, and of their sum: 2^e and the unscale factor stay normal numbers
static constexpr int ENC_POS_EXACT = 0x7fffffff;   // ec of a position that takes the all-exact kernels (a non-finite centroid)
static constexpr float ENC_EPS_ABS = 2e-34f;
__host__ __device__ inline float enc_eps_rel(int S) { return S <= 64 ? 2e-5f : S <= 320 ? 1.2e-4f : 2e-4f; }

typedef _Float16 ench8 __attribute__((ext_vector_type(8)));
typedef float encacc __attribute__((ext_vector_type(16)));

// Rows per chunk of a call: the candidate lists of a chunk are 136 bytes per item (116 MB at m = 12 with a coarse quantizer).
// Option encode_refine_all keeps every a: the chunk shrinks until [items][Kpad] floats stay within 512 MiB.
static inline int64_t enc_rows_per_chunk(int m, int Kpad, int Cpad, bool refine_all) {
  int64_t n = 1 << 16;
  if (refine_all) n = ((int64_t)512 << 20) / (int64_t)(sizeof(float) * ((size_t)m * Kpad + (size_t)Cpad));
  return n < 64 ? 64 : (n > (1 << 16) ? (1 << 16) : n);
}
// dynamic LDS of the filter kernel: the row fragments, seven words per row, the lists
static inline size_t enc_filter_lds(int T) { return (size_t)T * 256 * 16 + 7 * ENC_TQ * 4 + (size_t)ENC_TQ * ENC_CAP * 8; }

struct EncFilterArgs {
  const float* rows;        // [n][d] row-major: the chunk's rows
  const float* coarse;      // [C][d], or NULL: the rows themselves are searched
  const int32_t* cell;      // [n] the rows' cells (with coarse)
  int n, d, S, T, K, Kpad, npos;
  const ench8* img;         // [npos][Kpad / 32][T][2][64]
  const float* cn2;         // [npos][Kpad]
  const float* cmax;        // [npos]
  const int32_t* ec;        // [npos]
  float eps_rel;
  int32_t* cand_cnt;        // [n][npos]; -1: the item is in the redo list
  int32_t* cand_idx;        // [n][npos][ENC_KEEP]
  float* cand_a;            // [n][npos][ENC_KEEP]
  float* item_eps;          // [n][npos]
  int32_t* redo_cnt;        // [npos]
  int32_t* redo_rows;       // [npos][redo_stride]
  int redo_stride;
  float* all_a;             // NULL, or [n][npos][Kpad] (encode_refine_all)
};

template <int PF>
__global__ __launch_bounds__(256) void encode_filter_kernel(EncFilterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int p = blockIdx.x, row0 = blockIdx.y * ENC_TQ;
  const int T = a.T, S = a.S;
  ench8* frag = reinterpret_cast<ench8*>(smem);                       // [2][T][2][64]
  float* rown = reinterpret_cast<float*>(frag + (size_t)T * 256);     // [64] |x|^2
  float* runs = rown + ENC_TQ;                                        // [64] 2^-(ex + ec)
  float* reps = runs + ENC_TQ;                                        // [64] eps
  float* rsc = reps + ENC_TQ;                                         // [64] 2^ex
  uint32_t* Ub = reinterpret_cast<uint32_t*>(rsc + ENC_TQ);           // [64] bits of U
  int* cnt = reinterpret_cast<int*>(Ub + ENC_TQ);                     // [64] list lengths
  int* flag = cnt + ENC_TQ;                                           // [64] != 0: redo
  int* lidx = flag + ENC_TQ;                                          // [64][ENC_CAP]
  float* la = reinterpret_cast<float*>(lidx + ENC_TQ * ENC_CAP);      // [64][ENC_CAP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const float INF = __uint_as_float(0x7f800000u);
  const int ecp = a.ec[p];
  if (ecp == ENC_POS_EXACT) {   // the whole position takes the all-exact kernels
    if (tid < ENC_TQ && row0 + tid < a.n) {
      const int k = atomicAdd(a.redo_cnt + p, 1);
      a.redo_rows[(size_t)p * a.redo_stride + k] = row0 + tid;
      a.cand_cnt[(size_t)(row0 + tid) * a.npos + p] = -1;
    }
    return;
  }
  const ench8* imgp = a.img + (size_t)p * (a.Kpad >> 5) * T * 128;
  const float* cnp = a.cn2 + (size_t)p * a.Kpad;
  auto load_a = [&](int cb, int t, ench8& hi, ench8& lo) {
    const ench8* q = imgp + ((size_t)cb * T + t) * 128 + lane;
    hi = q[0];
    lo = q[64];
  };
  ench8 ph[PF], pl[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) load_a(wave, u < T ? u : T - 1, ph[u], pl[u]);

  // ---- the tile's rows: norms and scales (four threads per row), then the f16 fragments ----
  auto elem = [&](const float* x, const float* co, int j) -> float { return co ? x[j] - co[j] : x[j]; };   // (one rounded subtraction)
  {
    const int row = tid >> 2, part = tid & 3;
    const int gr = row0 + row < a.n ? row0 + row : a.n - 1;
    const float* x = a.rows + (size_t)gr * a.d + (size_t)p * S;
    const float* co = a.coarse ? a.coarse + (size_t)a.cell[gr] * a.d + (size_t)p * S : nullptr;
    float n2 = 0.0f, am = 0.0f;
    for (int j = part; j < S; j += 4) {
      const float v = elem(x, co, j);
      n2 = __builtin_fmaf(v, v, n2);
      am = fmaxf(am, __builtin_fabsf(v));
    }
    n2 += __shfl_xor(n2, 1, 64); am = fmaxf(am, __shfl_xor(am, 1, 64));
    n2 += __shfl_xor(n2, 2, 64); am = fmaxf(am, __shfl_xor(am, 2, 64));
    if (part == 0) {
      int e = 0;
      if (am > 0.0f && am < INF) { (void)__builtin_frexpf(am, &e); e = 14 - e; }
      const bool scale_ok = e >= -ENC_MAX_EXP && e <= ENC_MAX_EXP && e + ecp >= -ENC_MAX_EXP && e + ecp <= ENC_MAX_EXP;
      const float s = __builtin_sqrtf(n2) * (1.0f + 1e-6f) + a.cmax[p];
      const float eps = s * s * a.eps_rel + ENC_EPS_ABS;
      const bool ok = scale_ok && n2 < INF && eps < 1e30f;   // (false for NaN too)
      rown[row] = n2;
      rsc[row] = ok ? __builtin_ldexpf(1.0f, e) : 1.0f;
      runs[row] = ok ? __builtin_ldexpf(1.0f, -(e + ecp)) : 1.0f;
      reps[row] = ok ? eps : 0.0f;
      Ub[row] = 0x7f800000u;
      cnt[row] = 0;
      flag[row] = ok ? 0 : 1;
    }
  }
  __syncthreads();
  for (int i = tid; i < ENC_TQ * 2 * T; i += 256) {
    const int row = i / (2 * T), g8 = i - row * (2 * T);
    const int gr = row0 + row < a.n ? row0 + row : a.n - 1;
    const float* x = a.rows + (size_t)gr * a.d + (size_t)p * S;
    const float* co = a.coarse ? a.coarse + (size_t)a.cell[gr] * a.d + (size_t)p * S : nullptr;
    const float sc = rsc[row];
    ench8 hi, lo;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const int j = 8 * g8 + w;
      const float f = j < S ? elem(x, co, j < S ? j : 0) * sc : 0.0f;   // (a power of two: exact)
      const _Float16 hh = (_Float16)f;
      hi[w] = hh;
      lo[w] = (_Float16)(f - (float)hh);
    }
    const int t = g8 >> 1, g = g8 & 1, l = (row & 31) + 32 * g;
    frag[((size_t)((row >> 5) * T + t) * 2 + 0) * 64 + l] = hi;
    frag[((size_t)((row >> 5) * T + t) * 2 + 1) * 64 + l] = lo;
  }
  __syncthreads();

  const float xn0 = rown[r], xn1 = rown[32 + r];
  const float us0 = -2.0f * runs[r], us1 = -2.0f * runs[32 + r];   // (powers of two: -2 x.c exactly as accumulated)
  const float e0 = reps[r], e1 = reps[32 + r];
  const int nit = a.Kpad >> 7;
  for (int it = 0; it < nit; ++it) {
    const int cb = it * 4 + wave;
    encacc acc0, acc1;
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc0[v] = 0.0f; acc1[v] = 0.0f; }
    for (int t0 = 0; t0 < T; t0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int t = t0 + u;
        if (t < T) {
          const ench8 ch = ph[u], cl = pl[u];
          if (t + PF < T) load_a(cb, t + PF, ph[u], pl[u]);
          const ench8 b0h = frag[((size_t)t * 2 + 0) * 64 + lane], b0l = frag[((size_t)t * 2 + 1) * 64 + lane];
          const ench8 b1h = frag[((size_t)(T + t) * 2 + 0) * 64 + lane], b1l = frag[((size_t)(T + t) * 2 + 1) * 64 + lane];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, b0h, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, b1h, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, b0l, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, b1l, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, b0h, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, b1h, acc1, 0, 0, 0);
        }
      }
    }
    if (it + 1 < nit) {
#pragma unroll
      for (int u = 0; u < PF; ++u) load_a(cb + 4, u < T ? u : T - 1, ph[u], pl[u]);
    }
    // C layout of the 32 x 32 MFMA: register v of lane l holds result row 8 (v / 4) + 4 (l / 32) + v % 4 (a centroid), column l % 32 (a table row)
    const int cbase = cb * 32;
    float tv0[16], tv1[16];
    float mn0 = INF, mn1 = INF;
    bool bad0 = false, bad1 = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 cn4 = *reinterpret_cast<const float4*>(cnp + cbase + 8 * q + 4 * h);
      const float cn[4] = {cn4.x, cn4.y, cn4.z, cn4.w};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int v = 4 * q + w;
        const bool valid = cbase + 8 * q + 4 * h + w < a.K;
        float t0v = __builtin_fmaf(us0, acc0[v], xn0 + cn[w]);
        float t1v = __builtin_fmaf(us1, acc1[v], xn1 + cn[w]);
        if (!valid) { t0v = INF; t1v = INF; }
        else {
          if (!(__builtin_fabsf(t0v) < INF)) bad0 = true;
          if (!(__builtin_fabsf(t1v) < INF)) bad1 = true;
        }
        tv0[v] = t0v; tv1[v] = t1v;
        mn0 = fminf(mn0, t0v); mn1 = fminf(mn1, t1v);
      }
    }
    // a. lower U by the tile's minimum
    mn0 = fminf(mn0, __shfl_xor(mn0, 32, 64));
    mn1 = fminf(mn1, __shfl_xor(mn1, 32, 64));
    if (h == 0) {
      if (mn0 < INF) atomicMin(Ub + r, __float_as_uint(fmaxf(mn0 + e0, 0.0f)));
      if (mn1 < INF) atomicMin(Ub + 32 + r, __float_as_uint(fmaxf(mn1 + e1, 0.0f)));
    }
    if (bad0) flag[r] = 1;
    if (bad1) flag[32 + r] = 1;
    __syncthreads();
    // b. append the tile's centroids inside the bracket
    const float U0 = __uint_as_float(Ub[r]), U1 = __uint_as_float(Ub[32 + r]);
    const float Urow = tid < ENC_TQ ? __uint_as_float(Ub[tid]) : 0.0f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int c = cbase + 8 * (v >> 2) + 4 * h + (v & 3);
      if (tv0[v] < INF && tv0[v] - e0 <= U0) {
        const int slot = atomicAdd(cnt + r, 1);
        if (slot < ENC_CAP) { lidx[r * ENC_CAP + slot] = c; la[r * ENC_CAP + slot] = tv0[v]; }
      }
      if (tv1[v] < INF && tv1[v] - e1 <= U1) {
        const int slot = atomicAdd(cnt + 32 + r, 1);
        if (slot < ENC_CAP) { lidx[(32 + r) * ENC_CAP + slot] = c; la[(32 + r) * ENC_CAP + slot] = tv1[v]; }
      }
    }
    if (a.all_a) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int c = cbase + 8 * (v >> 2) + 4 * h + (v & 3);
        if (c < a.K && row0 + r < a.n) a.all_a[((size_t)(row0 + r) * a.npos + p) * a.Kpad + c] = tv0[v];
        if (c < a.K && row0 + 32 + r < a.n) a.all_a[((size_t)(row0 + 32 + r) * a.npos + p) * a.Kpad + c] = tv1[v];
      }
    }
    __syncthreads();
    // c. compaction against the U of step b
    if (tid < ENC_TQ && cnt[tid] > ENC_KEEP) {
      const int have = cnt[tid];
      const float eps = reps[tid];
      int k = 0;
      if (have > ENC_CAP) flag[tid] = 1;
      else {
        for (int i = 0; i < have; ++i) {
          const float av = la[tid * ENC_CAP + i];
          const int ci = lidx[tid * ENC_CAP + i];
          if (av - eps <= Urow) { lidx[tid * ENC_CAP + k] = ci; la[tid * ENC_CAP + k] = av; ++k; }
        }
        if (k > ENC_KEEP) { flag[tid] = 1; k = 0; }
      }
      cnt[tid] = k;
    }
  }
  // ---- the lists against the final U (the last tile's step b and c left them complete) ----
  if (tid < ENC_TQ && row0 + tid < a.n) {
    const size_t item = (size_t)(row0 + tid) * a.npos + p;
    if (flag[tid]) {
      const int k = atomicAdd(a.redo_cnt + p, 1);
      a.redo_rows[(size_t)p * a.redo_stride + k] = row0 + tid;
      a.cand_cnt[item] = -1;
    } else {
      const float U = __uint_as_float(Ub[tid]), eps = reps[tid];
      const int have = cnt[tid];
      int k = 0;
      for (int i = 0; i < have; ++i) {
        const float av = la[tid * ENC_CAP + i];
        if (av - eps <= U) { a.cand_idx[item * ENC_KEEP + k] = lidx[tid * ENC_CAP + i]; a.cand_a[item * ENC_KEEP + k] = av; ++k; }
      }
      a.cand_cnt[item] = k;
      a.item_eps[item] = eps;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Refine: one lane per item, the reference's chain for centroid 0 and the candidates.
// ---------------------------------------------------------------------------------------
struct EncRefineArgs {
  const float* rows;        // [n][d]
  const float* coarse;      // [C][d] or NULL
  const int32_t* cell;      // [n] (with coarse)
  const float* cent;        // [npos][K][S] row-major centroids
  int n, d, S, K, Kpad, npos;
  const int32_t* cand_cnt;
  const int32_t* cand_idx;
  const float* cand_a;
  const float* item_eps;
  const float* all_a;       // NULL, or every a: all K centroids are refined
  int32_t* out_cell;        // [n] (the coarse stage, npos == 1) or NULL
  int16_t* out_codes;       // [n][npos]
  unsigned long long* stats;   // [0] candidates refined, [1] brackets checked, [2] brackets violated
};

static __global__ __launch_bounds__(256) void encode_refine_kernel(EncRefineArgs a) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long n_cand = 0, n_chk = 0, n_viol = 0;
  if (item < (int64_t)a.n * a.npos) {
    const int cnt = a.cand_cnt[item];
    if (cnt >= 0) {
      const int row = (int)(item / a.npos), p = (int)(item - (int64_t)row * a.npos);
      const int S = a.S;
      const float* x = a.rows + (size_t)row * a.d + (size_t)p * S;
      const float* co = a.coarse ? a.coarse + (size_t)a.cell[row] * a.d + (size_t)p * S : nullptr;
      const float* cb = a.cent + (size_t)p * a.K * S;
      auto dist = [&](int c) -> float {   // index_utils.c:500-508: sub, mul, add rounded one by one, j ascending from +0
        const float* cv = cb + (size_t)c * S;
        float acc = 0.0f;
        for (int j = 0; j < S; ++j) {
          const float rj = co ? x[j] - co[j] : x[j];
          const float t = rj - cv[j];
          const float pr = t * t;
          acc = acc + pr;
        }
        return acc;
      };
      const float eps = a.item_eps[item];
      const float d0 = dist(0);
      u64 best = make_key(d0, 0u);
      const bool first_nan = d0 != d0;   // the search starts at centroid 0 and never leaves a NaN there
      const int n_ref = a.all_a ? a.K : cnt;
      for (int i = 0; i < n_ref; ++i) {
        const int c = a.all_a ? i : a.cand_idx[item * ENC_KEEP + i];
        const float ap = a.all_a ? a.all_a[(size_t)item * a.Kpad + c] : a.cand_a[item * ENC_KEEP + i];
        const float dd = c == 0 ? d0 : dist(c);
        best = umin64(best, make_key(dd, (uint32_t)c));
        ++n_chk;
        if (!(__builtin_fabsf(dd - ap) <= eps)) ++n_viol;
      }
      n_cand = (unsigned long long)n_ref;
      const int32_t win = first_nan ? 0 : (int32_t)key_pos(best);
      if (a.out_cell) a.out_cell[row] = win;
      else a.out_codes[(size_t)row * a.npos + p] = (int16_t)win;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_cand += __shfl_xor(n_cand, o, 64);
    n_chk += __shfl_xor(n_chk, o, 64);
    n_viol += __shfl_xor(n_viol, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_cand) atomicAdd(a.stats + 0, n_cand);
    if (n_chk) atomicAdd(a.stats + 1, n_chk);
    if (n_viol) atomicAdd(a.stats + 2, n_viol);
  }
}

// ---------------------------------------------------------------------------------------
// Redo: the listed rows of one position, compacted for the all-exact kernels, and their answers back.
// ---------------------------------------------------------------------------------------
// dst[i][0 .. S) = the sub-vector (residual) of position p of row list[i]
static __global__ __launch_bounds__(64) void encode_redo_gather_kernel(const float* __restrict__ rows, const float* __restrict__ coarse,
                                                                      const int32_t* __restrict__ cell, const int32_t* __restrict__ list,
                                                                      int count, int d, int S, int p, float* __restrict__ dst) {
  const int i = blockIdx.x;
  if (i >= count) return;
  const int row = list[i];
  const float* x = rows + (size_t)row * d + (size_t)p * S;
  const float* co = coarse ? coarse + (size_t)cell[row] * d + (size_t)p * S : nullptr;
  for (int j = threadIdx.x; j < S; j += 64) dst[(size_t)i * S + j] = co ? x[j] - co[j] : x[j];
}
// out_cell[list[i]] = cells[i]  /  out_codes[list[i]][p] = codes[i]
static __global__ __launch_bounds__(256) void encode_redo_scatter_kernel(const int32_t* __restrict__ list, int count, const int32_t* __restrict__ cells,
                                                                        const int16_t* __restrict__ codes, int m, int p,
                                                                        int32_t* __restrict__ out_cell, int16_t* __restrict__ out_codes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  if (cells) out_cell[list[i]] = cells[i];
  else out_codes[(size_t)list[i] * m + p] = codes[i];
}
// clears the chunk's redo counters (m + 1 words)
static __global__ __launch_bounds__(64) void encode_clear_kernel(int32_t* __restrict__ words, int n) {
  for (int i = threadIdx.x; i < n; i += 64) words[i] = 0;
}

}  // namespace freddy
