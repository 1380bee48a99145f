// assign_filter.h -- the assignment step of cluster_exact (assign.h: per target the first centroid under "similarity DESC in
// PostgreSQL's float4 order, centroid index ASC", similarity = the binary32 chain of cosine_similarity_bytea) as FILTER + REFINE on
// the matrix cores: option assign_filter of a vector handle; cluster.hip launches what is here for freddy_gpu_exact_assign and for
// freddy_gpu_cluster without a pq handle.  assign_exact_kernel evaluates the chain for EVERY (target, centroid) pair and keeps one
// argmax per target.  Here, per target x and centroid q:
//
//   a[q] = x.q on f16-SPLIT operands (v_mfma_f32_32x32x16_f16, fp32 accumulate): every fp32 input is hi + lo, hi = f16(v),
//          lo = f16(v - hi) after a power-of-two scaling; x.q ~ hi.hi + hi.lo + lo.hi
//
// with a proven bracket |a[q] - chain[q]| <= eps(x).  L = max_q (a[q] - eps) is a lower bound of the largest chain value, so the
// winner -- and every centroid that TIES with it -- has a[q] + eps >= L:
//   0. IMAGE   (assign_image_kernel, twice per set of centroids: once per call, once per round of the k-means): the centroids split
//              into the filter's A-fragment order ON THE DEVICE -- they are a kernel's output there, nothing waits for the host;
//   1. FILTER  (assign_filter_kernel): a for every centroid; the centroids with a + eps >= L are the target's candidates;
//   2. REFINE  (assign_refine_kernel): the reference's chain for the candidates in ascending index, a strictly larger assign_ord
//              replaces the best: the first of equal similarities wins, as in assign_exact_kernel;
//   3. REDO    (assign_redo_kernel): the targets the filter cannot answer, compacted on the device, through assign_exact_walk.inc,
//              the one copy of the all-exact loop (assign_exact_kernel's).
// The approximate value never reaches an output.
//
// The bracket (u = 2^-24; |.| Euclidean; d dimensions, T = ceil(d / 16) k-steps; P = sum_j |x_j q_j| <= |x||q|; E = sum_j x_j q_j):
//   reference chain   d products and d adds, each rounded once: |chain - E| <= ((1+u)^d - 1) P     d <= 64: 0.381e-5   320: 1.907e-5   512: 3.052e-5
//   dropped lo.lo     <= 2^-22 P;  lo rounded to f16 <= 2 * 2^-22 P (exact2.h, the same operands): 3 * 2^-22 P           0.072e-5
//                     (a lo, or a hi, that is subnormal in f16 is off by <= 2^-25 against a largest scaled element of >= 2^13:
//                     <= 2 * 2^-38 sqrt(d) |x| max|q| < 1e-10 |x| max|q|)
//   MFMA accumulation a product passes <= 16 in-step adds and the 3 T - 1 accumulations behind it, DOUBLED in case the matrix core
//                     truncates: 2 (3 T + 16) u (1 + 2^-10) P                                       d <= 64: 0.334e-5   320: 0.907e-5   512: 1.336e-5
//                     (the products of two f16 are exact in fp32; the unscaling is a multiplication by a power of two)
//   comparisons       the a - eps and a + eps of the filter: one rounding each, u (|a| + eps)                           0.012e-5
//   sum                                                                                           d <= 64: 0.80e-5    320: 2.90e-5    512: 4.47e-5
//   eps(x) = asf_eps_rel(d) xn max_q|q| + ENC_EPS_ABS,  asf_eps_rel = 2.5e-5 (d <= 64), 9e-5 (d <= 320), 1.4e-4 (d <= 512): 3.1x the sum.
//   xn >= |x|: the kernel's own |x|^2 is four fp32 fma chains of <= d / 4 + 1 terms, added: relative error (d / 4 + 4) u <= 0.79e-5,
//   half of it in the root, which is raised by 1e-5; squares that underflow are below 2^-149 each, d of them below the 2^-69 that is
//   added to the root.  max_q|q| from an fp64 sum, raised by 1e-6.  The product xn max|q| and the multiplication by asf_eps_rel round
//   twice (2u relative: inside the factor); where they underflow, what they stand for is below 2e-34.
// No overflow.  A target is only answered with eps < 1e30, so |x| max|q| < 1e35: every product and every partial sum of the
// reference's chain is below that -- the chain is a finite number and the bracket speaks about it.
// Small magnitudes.  Every operation whose result is subnormal is off by <= 2^-149 absolute instead of u relative: the 2 d of the
// chain and the unscaling, < 2e-42; ENC_EPS_ABS = 2e-34 covers them.  The unscale factor 2^-(ex + ec) may not underflow: a
// target whose scale exponents leave [-ENC_MAX_EXP, ENC_MAX_EXP] goes to the redo.
// The order.  assign_ord is monotone in the value (and puts +0 above -0): the centroids with the largest assign_ord have the
// largest chain value C >= L, so a + eps >= C >= L -- all of them are candidates, the first of them wins the refine.
// A target goes to the redo when (and only when)
//   - more than ENC_KEEP = 16 centroids lie inside the bracket of the running L at a tile boundary (below),
//   - its |x|^2, its eps or any a is not finite,
//   - its scale exponents leave the range above,
//   - or the image's flag is set (a non-finite centroid element, or a centroid scale outside the range): every target with a row.
// Which targets those are depends on the inputs alone.
//
// Layouts.  Qpad = Q rounded up to 128, T = ceil(d / 16).
//   img   [Qpad / 32][T][hi / lo][64 lanes][8 halves]: lane = centroid r + 32 g of the group of 32, its 8 values = dimensions
//         16 t + 8 g .. + 7, scaled by 2^ec, zeros beyond Q and d -- encode_filter.h's image.  ONE scale for all centroids.
//   head  AsfHead in front of it: the reduction words of the image's first launch, then ec, max|q| and the flag.
// assign_image_kernel, phase 0: a wave per centroid, lanes over the dimensions; the largest |element| (an unsigned maximum of the
// bits), the largest |q|^2 (fp64 per lane, added across the wave; an unsigned maximum of ITS bits) and "a non-finite element".
// Phase 1: a thread per (group, k-step, lane) writes its hi and lo operand; thread 0 derives ec, max|q| and the flag.
// assign_filter_kernel.  One workgroup of 256 threads per ASF_TQ = 64 targets (DESIGN.md 5.6d' has the LDS arithmetic that rules
// out 128 at d = 512).  Wave 0 resolves the ids (row_of_id, or cluster.h's row_of array).  Four threads per target take |x|^2 and
// the largest |element| with 16-byte loads; then the rows are split ONCE into LDS in B-fragment order [2 groups][T][hi / lo][64
// lanes] (the second read of a row comes from the cache).  The centroids stream by in tiles of 128: wave w owns centroids
// [128 i + 32 w, + 32) as the A operand and both target groups as B -- the centroids are the rows of the 32 x 32 result and the
// targets its columns, so the maximum over a wave's centroids is 15 in-lane v_max and one cross-half shuffle.  ENC_PF k-steps of A
// operands are in flight per wave; the next tile's first ones are requested before the epilogue.  Per tile:
//   a. every wave raises L[target] (LDS, atomicMax on assign_ord(max a - eps): order-preserving bits);
//   b. barrier; every lane appends its centroids with a + eps >= L[target] to the target's list (LDS, ENC_CAP = 32 slots);
//   c. barrier; a target with more than ENC_KEEP entries is compacted against the L of step b by ONE thread; still more than
//      ENC_KEEP -> redo.  More than ENC_CAP arrivals in one tile: the same rule.
// L only rises, every append of a tile sees the tile's own maximum, and the compaction reads the value step b read: the lists are
// the same SETS in every run.  At the end the list is filtered against the final L, sorted by index and written as (count,
// indices); count -1: the target is in the redo list; -2: the id has no row, (-1, -inf) is written here.
// assign_refine_kernel.  One lane per target, one wave per workgroup, dot_chain.h's gather tile for the 64 rows; every lane walks
// its own column against ITS candidates' centroids (read from [Q][d], which the caches hold), up to 16 accumulators.  Under the
// self-check (check_brackets bit 4) the filter keeps every a ([targets][Qpad]) and the refine walks all Q centroids, 16 at a time,
// comparing every bracket with the chain.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "assign.h"
#include "encode_filter.h"

namespace freddy {

static constexpr int ASF_TQ = 64;                  // targets per workgroup (two 32-column MFMA tiles)
static constexpr int ASF_CHECK = 16;               // check_brackets bit 4
static constexpr size_t ASF_ALL_BYTES = (size_t)512 << 20;   // the self-check's [targets][Qpad] floats per pass
__host__ __device__ inline float asf_eps_rel(int d) { return d <= 64 ? 2.5e-5f : d <= 320 ? 9e-5f : 1.4e-4f; }

struct AsfHead {              // 64 bytes in front of the image
  uint32_t amax_bits;         // phase 0: bits of the largest finite |element|
  uint32_t bad;               //          != 0: a non-finite element
  unsigned long long n2max_bits;   //     bits of the largest |q|^2 (fp64)
  int32_t ec;                 // phase 1: the centroids' scale exponent
  float cmax;                 //          max |q|, raised
  int32_t flag;               //          != 0: every target takes the redo
  int32_t redo_cnt;           // targets in the redo list of the pass
  unsigned long long stats[4];   // candidates refined, brackets checked, brackets violated, targets redone -- summed over the call
  unsigned long long filtered;   // targets with a row that entered the filter
};
static_assert(sizeof(AsfHead) == 72, "AsfHead");
static constexpr size_t ASF_HEAD_BYTES = 256;

static inline size_t asf_filter_lds(int T) { return (size_t)T * 256 * 16 + 7 * ASF_TQ * 4 + (size_t)ASF_TQ * ENC_CAP * 8; }
// targets per pass under the self-check: [targets][Qpad] floats stay within ASF_ALL_BYTES
static inline int64_t asf_check_pass(int Qpad) { return std::max<int64_t>(ASF_TQ, (int64_t)(ASF_ALL_BYTES / (sizeof(float) * (size_t)Qpad))); }

// the float whose assign_ord is o (o != 0xffffffff); o == 0 (nothing recorded) gives a NaN: every comparison with it fails
__device__ __forceinline__ float asf_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// before an image: clears the reduction words (and the call's counters when `first`); before every pass: the redo count
static __global__ __launch_bounds__(64) void assign_begin_kernel(AsfHead* h, int clear_image, int first) {
  if (threadIdx.x != 0) return;
  if (clear_image) { h->amax_bits = 0; h->bad = 0; h->n2max_bits = 0ull; }
  if (first) { h->stats[0] = h->stats[1] = h->stats[2] = h->stats[3] = 0ull; h->filtered = 0ull; }
  h->redo_cnt = 0;
}

struct AsfImageArgs {
  const float* queries;     // [Q][d]
  AsfHead* head;
  ench8* img;               // [Qpad / 32][T][2][64]
  int Q, Qpad, d, T, phase;
};

static __global__ __launch_bounds__(256) void assign_image_kernel(AsfImageArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (a.phase == 0) {
    for (int c = blockIdx.x * 4 + (tid >> 6); c < a.Q; c += gridDim.x * 4) {
      const float* q = a.queries + (size_t)c * a.d;
      double n2 = 0.0;
      float am = 0.0f;
      bool bad = false;
      for (int j = lane; j < a.d; j += 64) {
        const float v = q[j];
        const float av = __builtin_fabsf(v);
        if (!(av < __builtin_huge_valf())) bad = true;   // (NaN too)
        else am = fmaxf(am, av);
        n2 += (double)v * (double)v;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { n2 += __shfl_xor(n2, o, 64); am = fmaxf(am, __shfl_xor(am, o, 64)); }
      if (__ballot(bad) != 0ull) { if (lane == 0) atomicOr(&a.head->bad, 1u); }
      else if (lane == 0) {   // (non-negative numbers order as their bits)
        atomicMax(&a.head->amax_bits, __float_as_uint(am));
        atomicMax(&a.head->n2max_bits, (unsigned long long)__double_as_longlong(n2));
      }
    }
    return;
  }
  const float amax = __uint_as_float(a.head->amax_bits);
  int e = 0;
  if (amax > 0.0f) { (void)__builtin_frexpf(amax, &e); e = 14 - e; }
  const bool flag = a.head->bad != 0u || e < -ENC_MAX_EXP || e > ENC_MAX_EXP;
  if (flag) e = 0;   // (the image is not read then)
  if (blockIdx.x == 0 && tid == 0) {
    a.head->ec = e;
    a.head->cmax = (float)(__builtin_sqrt(__longlong_as_double((long long)a.head->n2max_bits)) * (1.0 + 1e-6));
    a.head->flag = flag ? 1 : 0;
  }
  const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
  if (idx >= (int64_t)(a.Qpad >> 5) * a.T * 64) return;
  const int t = (int)((idx >> 6) % a.T), cb = (int)((idx >> 6) / a.T);
  const int c = cb * 32 + (lane & 31), j0 = 16 * t + 8 * (lane >> 5);
  ench8 hi, lo;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const int j = j0 + w;
    float f = 0.0f;
    if (c < a.Q && j < a.d && !flag) f = __builtin_ldexpf(a.queries[(size_t)c * a.d + j], e);   // (a power of two: exact)
    const _Float16 hh = (_Float16)f;
    hi[w] = hh;
    lo[w] = (_Float16)(f - (float)hh);
  }
  ench8* dst = a.img + ((size_t)cb * a.T + t) * 128 + lane;
  dst[0] = hi;
  dst[64] = lo;
}

struct AsfFilterArgs {
  const int32_t* targets;   // [n] ids
  const int32_t* row_in;    // [n] their rows (cluster.h's row_of), or NULL: resolved here and written to row_out
  int32_t* row_out;         // [n] or NULL
  const int32_t* vec_ids;   // [N]
  const float* rows;        // [N][d]
  int64_t N;
  int n, d, T, Q, Qpad;
  AsfHead* head;
  const ench8* img;
  float eps_rel;
  int32_t* cand_cnt;        // [n]; -1: in the redo list, -2: no row
  int32_t* cand_idx;        // [n][ENC_KEEP] ascending
  float* tgt_eps;           // [n] (self-check)
  float* all_a;             // NULL, or [n][Qpad] (self-check)
  int32_t* redo_list;       // [n]
  int32_t* out_query;       // [n]: written here for ids without a row
  float* out_sim;
};

// eight consecutive elements of a row from dimension j (a multiple of 8), zeros from d on
__device__ __forceinline__ void asf_load8(const float* __restrict__ x, int j, int d, bool vec4, float (&v)[8]) {
  if (vec4) {   // d % 4 == 0: the rows are 16-byte aligned and no piece crosses the end
    const float4 p = j < d ? *reinterpret_cast<const float4*>(x + j) : float4{0.0f, 0.0f, 0.0f, 0.0f};
    const float4 q = j + 4 < d ? *reinterpret_cast<const float4*>(x + j + 4) : float4{0.0f, 0.0f, 0.0f, 0.0f};
    v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w; v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) v[w] = j + w < d ? x[j + w] : 0.0f;
  }
}

// the f16 split of eight elements scaled by sc (a power of two: exact): hi = f16(f), lo = f16(f - hi)
__device__ __forceinline__ void asf_split8(const float (&v)[8], float sc, ench8& hi, ench8& lo) {
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const float f = v[w] * sc;
    const _Float16 hh = (_Float16)f;
    hi[w] = hh;
    lo[w] = (_Float16)(f - (float)hh);
  }
}

template <int PF>
__global__ __launch_bounds__(256) void assign_filter_kernel(AsfFilterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char asf_smem[];
  const int row0 = blockIdx.x * ASF_TQ;
  const int T = a.T, d = a.d;
  ench8* frag = reinterpret_cast<ench8*>(asf_smem);                   // [2][T][2][64]
  int32_t* srow = reinterpret_cast<int32_t*>(frag + (size_t)T * 256); // [64] table rows
  float* runs = reinterpret_cast<float*>(srow + ASF_TQ);              // [64] 2^-(ex + ec)
  float* reps = runs + ASF_TQ;                                        // [64] eps
  float* rsc = reps + ASF_TQ;                                         // [64] 2^ex
  uint32_t* Lb = reinterpret_cast<uint32_t*>(rsc + ASF_TQ);           // [64] assign_ord of L
  int* cnt = reinterpret_cast<int*>(Lb + ASF_TQ);                     // [64] list lengths
  int* flag = cnt + ASF_TQ;                                           // [64] 1: redo, 2: no row
  int* lidx = flag + ASF_TQ;                                          // [64][ENC_CAP]
  float* la = reinterpret_cast<float*>(lidx + ASF_TQ * ENC_CAP);      // [64][ENC_CAP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const float INF = __builtin_huge_valf();
  const bool vec4 = (d & 3) == 0;

  if (tid < ASF_TQ) {
    const int i = row0 + tid;
    int32_t row = -1;
    if (i < a.n) {
      row = a.row_in ? a.row_in[i] : row_of_id(a.vec_ids, a.N, a.targets[i]);
      if (a.row_out) a.row_out[i] = row;
    }
    srow[tid] = row;
    const unsigned long long have = __ballot(row >= 0);
    if (tid == 0 && have) atomicAdd(&a.head->filtered, (unsigned long long)__popcll(have));
  }
  const bool img_exact = a.head->flag != 0;
  const int ecp = a.head->ec;
  const float cmax = a.head->cmax;
  __syncthreads();
  if (img_exact) {   // every target with a row takes the all-exact walk
    if (tid < ASF_TQ && row0 + tid < a.n) {
      const int i = row0 + tid;
      if (srow[tid] >= 0) { a.redo_list[atomicAdd(&a.head->redo_cnt, 1)] = i; a.cand_cnt[i] = -1; }
      else { a.cand_cnt[i] = -2; a.out_query[i] = -1; a.out_sim[i] = -INF; }
    }
    return;
  }
  auto load_a = [&](int cb, int t, ench8& hi, ench8& lo) {
    const ench8* q = a.img + ((size_t)cb * T + t) * 128 + lane;
    hi = q[0];
    lo = q[64];
  };
  ench8 ph[PF], pl[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) load_a(wave, u < T ? u : T - 1, ph[u], pl[u]);

  // ---- the tile's rows: norms and scales (four threads per target), then the f16 fragments ----
  {
    const int row = tid >> 2, part = tid & 3;
    const int32_t gr = srow[row];
    float n2 = 0.0f, am = 0.0f;
    if (gr >= 0) {
      const float* x = a.rows + (size_t)gr * d;
      if (vec4) {
        for (int j = 4 * part; j < d; j += 16) {
          const float4 v = *reinterpret_cast<const float4*>(x + j);
          n2 = __builtin_fmaf(v.x, v.x, n2); n2 = __builtin_fmaf(v.y, v.y, n2); n2 = __builtin_fmaf(v.z, v.z, n2); n2 = __builtin_fmaf(v.w, v.w, n2);
          am = fmaxf(fmaxf(am, fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y))), fmaxf(__builtin_fabsf(v.z), __builtin_fabsf(v.w)));
        }
      } else {
        for (int j = part; j < d; j += 4) {
          const float v = x[j];
          n2 = __builtin_fmaf(v, v, n2);
          am = fmaxf(am, __builtin_fabsf(v));
        }
      }
    }
    n2 += __shfl_xor(n2, 1, 64); am = fmaxf(am, __shfl_xor(am, 1, 64));
    n2 += __shfl_xor(n2, 2, 64); am = fmaxf(am, __shfl_xor(am, 2, 64));
    if (part == 0) {
      int e = 0;
      if (am > 0.0f && am < INF) { (void)__builtin_frexpf(am, &e); e = 14 - e; }
      const bool scale_ok = e >= -ENC_MAX_EXP && e <= ENC_MAX_EXP && e + ecp >= -ENC_MAX_EXP && e + ecp <= ENC_MAX_EXP;
      const float xn = __builtin_sqrtf(n2) * (1.0f + 1e-5f) + 0x1p-69f;
      const float eps = a.eps_rel * (xn * cmax) + ENC_EPS_ABS;
      const bool ok = scale_ok && n2 < INF && eps < 1e30f;   // (false for NaN too)
      rsc[row] = ok ? __builtin_ldexpf(1.0f, e) : 1.0f;
      runs[row] = ok ? __builtin_ldexpf(1.0f, -(e + ecp)) : 1.0f;
      reps[row] = ok ? eps : 0.0f;
      Lb[row] = 0u;
      cnt[row] = 0;
      flag[row] = gr < 0 ? 2 : (ok ? 0 : 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < ASF_TQ * 2 * T; i += 256) {
    const int row = i / (2 * T), g8 = i - row * (2 * T);
    const int32_t gr = srow[row];
    float v[8];
    if (gr >= 0 && flag[row] == 0) asf_load8(a.rows + (size_t)gr * d, 8 * g8, d, vec4, v);
    else {
#pragma unroll
      for (int w = 0; w < 8; ++w) v[w] = 0.0f;
    }
    const float sc = rsc[row];
    ench8 hi, lo;
    asf_split8(v, sc, hi, lo);
    const int t = g8 >> 1, g = g8 & 1, l = (row & 31) + 32 * g;
    frag[((size_t)((row >> 5) * T + t) * 2 + 0) * 64 + l] = hi;
    frag[((size_t)((row >> 5) * T + t) * 2 + 1) * 64 + l] = lo;
  }
  __syncthreads();

  const float us0 = runs[r], us1 = runs[32 + r];   // (powers of two)
  const float e0 = reps[r], e1 = reps[32 + r];
  const int nit = a.Qpad >> 7;
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
    // C layout of the 32 x 32 MFMA: register v of lane l holds result row 8 (v / 4) + 4 (l / 32) + v % 4 (a centroid), column l % 32 (a target)
    const int cbase = cb * 32;
    float tv0[16], tv1[16];
    float mx0 = -INF, mx1 = -INF;
    bool bad0 = false, bad1 = false;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const bool valid = cbase + 8 * (v >> 2) + 4 * h + (v & 3) < a.Q;
      float t0v = acc0[v] * us0, t1v = acc1[v] * us1;
      if (!valid) { t0v = -INF; t1v = -INF; }
      else {
        if (!(__builtin_fabsf(t0v) < INF)) bad0 = true;
        if (!(__builtin_fabsf(t1v) < INF)) bad1 = true;
      }
      tv0[v] = t0v; tv1[v] = t1v;
      mx0 = fmaxf(mx0, t0v); mx1 = fmaxf(mx1, t1v);
    }
    // a. raise L by the tile's maximum
    mx0 = fmaxf(mx0, __shfl_xor(mx0, 32, 64));
    mx1 = fmaxf(mx1, __shfl_xor(mx1, 32, 64));
    if (h == 0) {
      if (mx0 > -INF) atomicMax(Lb + r, assign_ord(mx0 - e0));
      if (mx1 > -INF) atomicMax(Lb + 32 + r, assign_ord(mx1 - e1));
    }
    if (bad0) flag[r] |= 1;
    if (bad1) flag[32 + r] |= 1;
    __syncthreads();
    // b. append the tile's centroids inside the bracket
    const float L0 = asf_unord(Lb[r]), L1 = asf_unord(Lb[32 + r]);
    const float Lrow = tid < ASF_TQ ? asf_unord(Lb[tid]) : 0.0f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int c = cbase + 8 * (v >> 2) + 4 * h + (v & 3);
      if (tv0[v] > -INF && tv0[v] + e0 >= L0) {
        const int slot = atomicAdd(cnt + r, 1);
        if (slot < ENC_CAP) { lidx[r * ENC_CAP + slot] = c; la[r * ENC_CAP + slot] = tv0[v]; }
      }
      if (tv1[v] > -INF && tv1[v] + e1 >= L1) {
        const int slot = atomicAdd(cnt + 32 + r, 1);
        if (slot < ENC_CAP) { lidx[(32 + r) * ENC_CAP + slot] = c; la[(32 + r) * ENC_CAP + slot] = tv1[v]; }
      }
    }
    if (a.all_a) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int c = cbase + 8 * (v >> 2) + 4 * h + (v & 3);
        if (c < a.Q && row0 + r < a.n) a.all_a[(size_t)(row0 + r) * a.Qpad + c] = tv0[v];
        if (c < a.Q && row0 + 32 + r < a.n) a.all_a[(size_t)(row0 + 32 + r) * a.Qpad + c] = tv1[v];
      }
    }
    __syncthreads();
    // c. compaction against the L of step b
    if (tid < ASF_TQ && cnt[tid] > ENC_KEEP) {
      const int have = cnt[tid];
      const float eps = reps[tid];
      int k = 0;
      if (have > ENC_CAP) flag[tid] |= 1;
      else {
        for (int i = 0; i < have; ++i) {
          const float av = la[tid * ENC_CAP + i];
          const int ci = lidx[tid * ENC_CAP + i];
          if (av + eps >= Lrow) { lidx[tid * ENC_CAP + k] = ci; la[tid * ENC_CAP + k] = av; ++k; }
        }
        if (k > ENC_KEEP) { flag[tid] |= 1; k = 0; }
      }
      cnt[tid] = k;
    }
  }
  // ---- the lists against the final L (the last tile's steps b and c left them complete), in ascending index ----
  if (tid < ASF_TQ && row0 + tid < a.n) {
    const int i = row0 + tid;
    if (flag[tid] & 2) { a.cand_cnt[i] = -2; a.out_query[i] = -1; a.out_sim[i] = -INF; }
    else if (flag[tid]) { a.redo_list[atomicAdd(&a.head->redo_cnt, 1)] = i; a.cand_cnt[i] = -1; }
    else {
      const float L = asf_unord(Lb[tid]), eps = reps[tid];
      const int have = cnt[tid];
      int* li = lidx + tid * ENC_CAP;
      int k = 0;
      for (int s = 0; s < have; ++s) {
        if (!(la[tid * ENC_CAP + s] + eps >= L)) continue;
        const int c = li[s];   // (insertion into the sorted front: k <= s, the slot read is never overwritten before)
        int p = k++;
        for (; p > 0 && li[p - 1] > c; --p) li[p] = li[p - 1];
        li[p] = c;
      }
      for (int s = 0; s < k; ++s) a.cand_idx[(size_t)i * ENC_KEEP + s] = li[s];
      a.cand_cnt[i] = k;
      if (a.tgt_eps) a.tgt_eps[i] = eps;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Refine: one lane per target, the reference's chain for its candidates in ascending index.
// ---------------------------------------------------------------------------------------
struct AsfRefineArgs {
  const int32_t* trow;      // [n] table rows of the targets
  const float* rows;        // [N][d]
  const float* queries;     // [Q][d]
  int n, d, Q, Qpad;
  const int32_t* cand_cnt;
  const int32_t* cand_idx;
  const float* tgt_eps;     // (self-check)
  const float* all_a;       // NULL, or every a: all Q centroids are refined and every bracket is checked
  int32_t* out_query;
  float* out_sim;
  AsfHead* head;
  int32_t* viol;            // the handle's self-check words ([0] += violated, [1] += checked), with all_a
};

static __global__ __launch_bounds__(64) void assign_refine_kernel(AsfRefineArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_FLOATS];     // [TILE_DCH][TILE_STRIDE]
  const int lane = threadIdx.x, d = a.d;
  const int i = blockIdx.x * 64 + lane;
  const int cnt = i < a.n ? a.cand_cnt[i] : -2;
  const int32_t row = cnt >= 0 ? a.trow[i] : -1;
  const int n_ref = cnt < 0 ? 0 : (a.all_a ? a.Q : cnt);
  int n_max = n_ref;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_max = max(n_max, __shfl_xor(n_max, o, 64));
  const bool vec4 = (d & 3) == 0;
  const float eps = (a.all_a && cnt >= 0) ? a.tgt_eps[i] : 0.0f;
  uint32_t best_ord = 0;
  int32_t best_q = -1;
  float best_sim = -__builtin_huge_valf();
  unsigned n_chk = 0, n_viol = 0;
  for (int base = 0; base < n_max; base += ENC_KEEP) {
    const int kmax = min(ENC_KEEP, n_max - base);   // (the same in every lane)
    int cq[ENC_KEEP];
    float acc[ENC_KEEP];
#pragma unroll
    for (int k = 0; k < ENC_KEEP; ++k) {
      acc[k] = 0.0f;
      cq[k] = base + k < n_ref ? (a.all_a ? base + k : a.cand_idx[(size_t)i * ENC_KEEP + k]) : 0;   // (centroid 0 stands in: its value is not used)
    }
    for (int c0 = 0; c0 < d; c0 += TILE_DCH) {
      const int nd = (d - c0 < TILE_DCH) ? d - c0 : TILE_DCH;
      float4 v[8];
#pragma unroll
      for (int it = 0; it < 8; ++it) v[it] = tile_row_piece(a.rows, row, it, lane, d, c0, nd, vec4);
#pragma unroll
      for (int it = 0; it < 8; ++it) tile_store_row_piece(tile, v[it], it, lane);
      wave_lds_sync();
#pragma unroll
      for (int k = 0; k < ENC_KEEP; ++k)
        if (k < kmax) chain1<1, TILE_STRIDE>(acc[k], a.queries + (size_t)cq[k] * d + c0, tile + lane, nd);
      wave_lds_sync();
    }
#pragma unroll
    for (int k = 0; k < ENC_KEEP; ++k) {
      if (base + k >= n_ref) continue;
      const uint32_t o = assign_ord(acc[k]);
      if (o > best_ord) { best_ord = o; best_q = cq[k]; best_sim = acc[k]; }
      if (a.all_a) {
        ++n_chk;
        if (!(__builtin_fabsf(acc[k] - a.all_a[(size_t)i * a.Qpad + cq[k]]) <= eps)) ++n_viol;
      }
    }
  }
  if (cnt >= 0) { a.out_query[i] = best_q; a.out_sim[i] = best_sim; }
  unsigned n_cand = (unsigned)n_ref;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_cand += __shfl_xor(n_cand, o, 64);
    n_chk += __shfl_xor(n_chk, o, 64);
    n_viol += __shfl_xor(n_viol, o, 64);
  }
  if (lane == 0) {
    if (n_cand) atomicAdd(a.head->stats + 0, (unsigned long long)n_cand);
    if (n_chk) { atomicAdd(a.head->stats + 1, (unsigned long long)n_chk); atomicAdd(a.viol + 1, (int)n_chk); }
    if (n_viol) { atomicAdd(a.head->stats + 2, (unsigned long long)n_viol); atomicAdd(a.viol + 0, (int)n_viol); }
  }
}

// ---------------------------------------------------------------------------------------
// Redo: the listed targets, 64 per workgroup, through the all-exact walk (assign_exact_walk.inc).  The grid is sized for the whole pass; a workgroup whose
// slots lie beyond the device's count leaves at once -- the host never learns the count between two launches.
// ---------------------------------------------------------------------------------------
struct AsfRedoArgs {
  const int32_t* redo_list;
  const int32_t* trow;
  const float* rows;
  const float* queries;
  int d, Q;
  int32_t* out_query;
  float* out_sim;
  AsfHead* head;
};

static __global__ __launch_bounds__(64) void assign_redo_kernel(AsfRedoArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_FLOATS];
  __shared__ __attribute__((aligned(16))) float qs[TILE_QFLOATS];
  const int count = a.head->redo_cnt;
  const int lane = threadIdx.x, slot = blockIdx.x * 64 + lane, d = a.d;
  if ((int)blockIdx.x * 64 >= count) return;
  if (slot == 0) atomicAdd(a.head->stats + 3, (unsigned long long)count);
  const int i = slot < count ? a.redo_list[slot] : -1;
  const int32_t row = i >= 0 ? a.trow[i] : -1;
#include "assign_exact_walk.inc"
  if (i >= 0) { a.out_query[i] = best_q; a.out_sim[i] = best_sim; }
}

}  // namespace freddy
