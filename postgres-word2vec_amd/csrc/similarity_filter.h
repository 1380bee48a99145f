// similarity_filter.h -- the join "WHERE cosine_similarity(a, b) > t" (similarity.h: freddy_gpu_similarity_join) as FILTER + REFINE on
// the matrix cores: option similarity_filter of a vector handle; similarity.hip launches what is here.  sim_matrix_kernel evaluates the
// reference's chain for EVERY (A row, B row) pair of a pass so that the few pairs above t can leave the device.  Here, per pass:
//
//   1. IMAGE   (simf_image_kernel): the pass's A rows (w_q: gathered by id or staged from the caller's floats) split ON THE DEVICE into
//              f16 hi / lo in MFMA A-fragment order, ONE power-of-two scale 2^ea for the pass; max_i |a_i|; a flag per unfit row;
//   2. FILTER  (simf_filter_kernel, v_mfma_f32_32x32x16_f16): a = a_i.b_j ~ hi.hi + hi.lo + lo.hi, fp32 accumulate, for every pair; bit
//              (i, j) of the candidate bitmap is set iff both rows are known and (the pair is unfit or a + eps(j) >= t);
//   3. LIST    (simf_count_kernel, sim_scan_kernel, simf_list_kernel): the bitmap's set bits as (i, j), i ascending then j ascending;
//   4. REFINE  (simf_refine_kernel): the reference's chain for every candidate, then sim_float4gt(chain, t); the matches are
//              compacted in list order (simf_count_kernel on the flags, sim_scan_kernel, simf_out_kernel).
// The approximate value never reaches an output: every (i, j, sim) written is a chain value that passed PostgreSQL's float4gt, and
// every pair whose chain passes it is a candidate (below), so the triples, their order and the total are today's.
//
// The bracket (assign_filter.h proves it for ONE scale of the whole image; u = 2^-24, d dimensions, T = ceil(d / 16) k-steps):
//   |a - chain| <= eps(j) = asf_eps_rel(d) bn_j max_i an_i + ENC_EPS_ABS        an_i >= |a_i|, bn_j >= |b_j|
// with the terms of assign_filter.h's table (the chain's d roundings, the dropped lo.lo and the rounded lo, the MFMA accumulation
// doubled, the comparison's rounding -- here ONE fma, a us + eps, and the compare) and its sum: 0.80e-5 (d <= 64), 2.90e-5 (320),
// 4.47e-5 (512) against asf_eps_rel = 2.5e-5 / 9e-5 / 1.4e-4.  It does NOT hold with an_i in place of max_i an_i: a half that goes
// subnormal in f16 is off by 2^-25 of the IMAGE's largest scaled element, not of row i's -- a row 2^-28 times smaller than its
// neighbours loses its lo and most of its hi (tests/test_similarity_filter_cpu.py constructs the violation).  The per-pass maximum costs
// nothing on a normalised table.
//   The B side is read ONCE (3.6 GB at 3 M x 300) and split in registers, so its scale must be known before its first element: every B
//   row takes the PASS's scale 2^eb, eb = ea - 1 (the A image's largest element lands in [2^13, 2^14); a B element may be up to four
//   times larger).  What that costs is a window.  A B element f = b 2^eb with |f| <= 2^15 has a normal or subnormal hi and a lo with
//   |f - hi - lo| <= max(2^-22 |f|, 2^-25) (the second where lo is subnormal in f16).  The first is the table's "lo rounded" term.  The
//   second adds, unscaled, at most 2^-25 2^-eb sum_k |a_ik| <= 2^-25 2^-eb sqrt(512) |a_i| < 0.0675 2^-eb max_i an_i to |a - chain|;
//   with bn_j >= 2^-(eb + 3), i.e. 2^-eb <= 8 bn_j, that is < 0.54e-5 bn_j max_i an_i, and the sums become 1.34e-5 / 3.44e-5 / 5.01e-5:
//   still 1.8x to 2.8x below asf_eps_rel.
//   bn_j = sqrt(n2) (1 + 2e-5) + 2^-69: n2 is one fp32 fma chain of <= 256 squares per half-wave lane, the two added: relative error
//   <= 258 u = 1.54e-5, half of it in the root; squares that underflow are below 2^-149 each.  max_i an_i: an fp64 sum, raised by 1e-6.
// Unfit, as a function of the inputs alone.  An A row: a non-finite element; every A row of a pass whose scale exponents leave
// [-ENC_MAX_EXP, ENC_MAX_EXP] (ea, eb or ea + eb).  A B row: n2 or eps not finite, eps >= 1e30 (no overflow: assign_filter.h), a largest
// |element| above 2^(15 - eb), or sqrt(n2) < 2^-(eb + 3) unless every element is zero (then a = chain = +-0 and nothing was rounded).
// A pair with an unfit row is ALWAYS a candidate: it gets the chain, so NaN, overflow, 2^60 and 2^-60 behave as today with no redo kernel.
// A fit pair with chain > t has a + eps >= chain > t: a candidate.  t = NaN: no comparison holds, no fit bit; t = -inf: every fit bit;
// t = +inf: no fit bit (a fit pair's chain is finite) -- only the unfit pairs' NaNs can match, as today.
//
// Layouts.  n rows in the pass, tiles = ceil(n / 32), W = ceil(nb / 32).
//   img     [tiles][T][hi / lo][64 lanes][8 halves]: lane = row r + 32 g of the tile, its 8 values = dimensions 16 t + 8 g .. + 7 scaled by
//           2^ea; zeros for rows that are unknown, unfit or beyond n, and beyond d.
//   amask   [tiles][2] 32-bit words: bit r of word 0 = row known, of word 1 = row unfit.
//   bitmap  [tiles * 32][W] words: bit c of word (i, s) = pair (i, 32 s + c).
// simf_filter_kernel.  512 threads; blockIdx.y owns AT consecutive A tiles (template: 1, 2), copied once into LDS -- AT T 2 KiB:
//   d = 300 (T = 19): 2 tiles = 77 824 B;  d = 512 (T = 32): 2 tiles = 131 072 B.  By LDS that is two workgroups per CU at d = 300 and one
//   at d = 512; by registers (224 at two tiles: two waves per SIMD) it is one workgroup of 8 waves per CU either way, two with one tile
//   (125 registers).  After that one barrier the waves share nothing.  A wave takes strips of 32 B rows
//   (blockIdx.x * 8 + wave, strided by the grid): lane l owns B row 32 s + l % 32 and the dimensions 16 t + 8 (l / 32) .. + 7 -- the B
//   operand of the 32 x 32 x 16 instruction as it stands, two 16-byte loads per k-step (simf_load8), SIMF_PF = 2 k-steps requested ahead.  n2
//   and the largest |element| accumulate from the same registers; the split (asf_split8) happens in registers; per k-step and A tile
//   three matrix instructions against the tile's hi / lo from LDS, AT accumulators of 16 registers.  No LDS and no barrier for B.
//   Epilogue, per accumulator register v (result row 8 (v / 4) + 4 (l / 32) + v % 4, column l % 32): one fma, one compare, one ballot;
//   the ballot's halves are two A rows x 32 B rows; lane r < 32 keeps the word of row r and stores it -- no atomics.
// simf_refine_kernel: sim_pairs_kernel's two gather tiles with the A rows taken from w_q by row number; one lane per candidate.
// Under the self-check (check_brackets bit 5) the filter also keeps every a, eps(j) and "B row j is fit"; sim_matrix_kernel computes the
// chain of every pair of the pass and simf_check_kernel compares every known fit pair.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "similarity.h"
#include "assign_filter.h"

namespace freddy {

static constexpr int SIMF_CHECK = 32;              // check_brackets bit 5
static constexpr int SIMF_MIN_D = 16;              // below: one k-step would be mostly padding; above ENC_MAX_S the bracket is not proven
static constexpr int SIMF_PF = 2;                  // k-steps of a B row requested ahead per lane (2 x 32 B)
static constexpr int SIMF_WAVES = 8;               // waves per workgroup of the filter
static constexpr int SIMF_MAX_AT = 2;              // A tiles of 32 rows per workgroup (four: 256 registers and scratch, DESIGN.md 5.6e')
static constexpr size_t SIMF_LDS = (size_t)160 << 10;
static constexpr int64_t SIMF_PASS_PAIRS = (int64_t)1 << 30;   // pairs per pass at most: a pass's counts are 32-bit numbers
static constexpr int SIMF_CAND_BYTES = 20;         // list bytes per candidate: i, j, value, flag, scanned offset
// Value 1 hands a pass to sim_matrix_kernel when more than 1 / SIMF_DENSE_DIV of its known pairs are candidates: the measured
// crossover density halved: value 2 wins at 1 % and loses at 10 % of the pairs at 100 x 3 M and at 4096 x 4096, 10 % / 2 = 1 / 20
// (profiles/similarity_filter_timing.txt, DESIGN.md 5.6e').
static constexpr int SIMF_DENSE_DIV = 20;

static inline int simf_tiles_per_wg(int T, int n_tiles) {
  int at = SIMF_MAX_AT;
  while (at > 1 && ((size_t)at * T * 2048 > SIMF_LDS || at / 2 >= n_tiles)) at /= 2;
  return at;
}

struct SimfHead {             // 64 bytes
  uint32_t amax_bits;         // phase 0: bits of the largest |element| of the known, finite A rows
  uint32_t known_b;           // known B ids of the call (simf_known_kernel)
  unsigned long long n2max_bits;   //     bits of their largest |a|^2 (fp64)
  int32_t ea;                 // phase 1: the pass's scale exponent
  float amaxn;                //          max_i an_i, raised
  int32_t flag;               //          != 0: the scale exponents leave the range, every row is unfit
  int32_t pad[9];
};
static_assert(sizeof(SimfHead) == 64, "SimfHead");

// before a pass: the reduction words
static __global__ __launch_bounds__(64) void simf_begin_kernel(SimfHead* h, int first) {
  if (threadIdx.x != 0) return;
  h->amax_bits = 0; h->n2max_bits = 0ull;
  if (first) h->known_b = 0;
}

// once per call: the number of known B ids
static __global__ __launch_bounds__(256) void simf_known_kernel(const uint8_t* __restrict__ known, int n, SimfHead* h) {
  unsigned c = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) c += known[i] ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&h->known_b, c);
}

struct SimfImageArgs {
  const float* a;           // [n][d] the pass's A rows
  const uint8_t* known_a;   // [n], or NULL: all known
  SimfHead* head;
  uint8_t* row_flag;        // [tiles * 32] bit 0: known, bit 1: unfit (phase 0 writes, phase 1 reads)
  uint32_t* amask;          // [tiles][2]
  ench8* img;               // [tiles][T][2][64]
  int n, tiles, d, T, phase;
};

static __global__ __launch_bounds__(256) void simf_image_kernel(SimfImageArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (a.phase == 0) {   // a wave per row, lanes over the dimensions
    for (int c = blockIdx.x * 4 + (tid >> 6); c < a.tiles * 32; c += gridDim.x * 4) {
      const bool known = c < a.n && (a.known_a == nullptr || a.known_a[c] != 0);
      double n2 = 0.0;
      float am = 0.0f;
      bool bad = false;
      if (known) {
        const float* q = a.a + (size_t)c * a.d;
        for (int j = lane; j < a.d; j += 64) {
          const float v = q[j];
          const float av = __builtin_fabsf(v);
          if (!(av < __builtin_huge_valf())) bad = true;   // (NaN too)
          else am = fmaxf(am, av);
          n2 += (double)v * (double)v;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { n2 += __shfl_xor(n2, o, 64); am = fmaxf(am, __shfl_xor(am, o, 64)); }
      const bool unfit = __ballot(bad) != 0ull;
      if (lane == 0) {
        a.row_flag[c] = (uint8_t)((known ? 1 : 0) | (unfit ? 2 : 0));
        if (known && !unfit) {   // (non-negative numbers order as their bits)
          atomicMax(&a.head->amax_bits, __float_as_uint(am));
          atomicMax(&a.head->n2max_bits, (unsigned long long)__double_as_longlong(n2));
        }
      }
    }
    return;
  }
  const float amax = __uint_as_float(a.head->amax_bits);
  int e = 0;
  if (amax > 0.0f) { (void)__builtin_frexpf(amax, &e); e = 14 - e; }
  const bool flag = e < -ENC_MAX_EXP || e > ENC_MAX_EXP || 2 * e - 1 < -ENC_MAX_EXP || 2 * e - 1 > ENC_MAX_EXP;
  if (flag) e = 0;
  if (blockIdx.x == 0 && tid == 0) {
    a.head->ea = e;
    a.head->amaxn = (float)(__builtin_sqrt(__longlong_as_double((long long)a.head->n2max_bits)) * (1.0 + 1e-6));
    a.head->flag = flag ? 1 : 0;
  }
  const int64_t idx = (int64_t)blockIdx.x * 256 + tid;   // (a wave = one (tile, k-step))
  if (idx >= (int64_t)a.tiles * a.T * 64) return;
  const int t = (int)((idx >> 6) % a.T), cb = (int)((idx >> 6) / a.T);
  const int c = cb * 32 + (lane & 31), j0 = 16 * t + 8 * (lane >> 5);
  const uint8_t rf = a.row_flag[c];
  if (t == 0) {
    const unsigned long long km = __ballot((rf & 1) != 0), um = __ballot(flag || (rf & 2) != 0);
    if (lane == 0) { a.amask[2 * cb] = (uint32_t)km; a.amask[2 * cb + 1] = (uint32_t)um; }
  }
  float v[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) v[w] = (rf == 1 && !flag && j0 + w < a.d) ? a.a[(size_t)c * a.d + j0 + w] : 0.0f;
  ench8 hi, lo;
  asf_split8(v, __builtin_ldexpf(1.0f, e), hi, lo);
  ench8* dst = a.img + ((size_t)cb * a.T + t) * 128 + lane;
  dst[0] = hi;
  dst[64] = lo;
}

struct SimfFilterArgs {
  const int32_t* b_rows;    // [nb] rows of the B ids, -1: none (sim_rows_kernel)
  const float* rows;        // [N][d] the table
  const ench8* img;
  const SimfHead* head;
  const uint32_t* amask;    // [tiles][2]
  uint32_t* bitmap;         // [tiles * 32][W]
  float* all_a;             // NULL, or [tiles * 32][nb] (self-check)
  float* b_eps;             // [nb] (self-check)
  uint8_t* b_fit;           // [nb] (self-check)
  int n, tiles, nb, W, d, T;
  float eps_rel, threshold;
};

// Eight consecutive elements of a table row from dimension j (a multiple of 8), zeros from d on and for a B id without a row (live =
// false; x is row 0 then) -- asf_load8 without a branch: j differs between the halves of the wave, so every guarded load would be a
// divergent region with its saved exec mask (scalar registers that spill).  The address is clamped into the row, the value selected.
__device__ __forceinline__ void simf_load8(const float* __restrict__ x, int j, int d, bool live, bool vec4, float (&v)[8]) {
  if (vec4) {   // d % 4 == 0, d >= 16: the rows are 16-byte aligned and no piece crosses the end
    const float4 p = *reinterpret_cast<const float4*>(x + (j < d ? j : d - 4));
    const float4 q = *reinterpret_cast<const float4*>(x + (j + 4 < d ? j + 4 : d - 4));
    const bool k0 = live && j < d, k1 = live && j + 4 < d;
    v[0] = k0 ? p.x : 0.0f; v[1] = k0 ? p.y : 0.0f; v[2] = k0 ? p.z : 0.0f; v[3] = k0 ? p.w : 0.0f;
    v[4] = k1 ? q.x : 0.0f; v[5] = k1 ? q.y : 0.0f; v[6] = k1 ? q.z : 0.0f; v[7] = k1 ? q.w : 0.0f;
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const float f = x[j + w < d ? j + w : d - 1];
      v[w] = (live && j + w < d) ? f : 0.0f;
    }
  }
}

template <int AT, bool VEC4>
__global__ __launch_bounds__(SIMF_WAVES * 64) void simf_filter_kernel(SimfFilterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char simf_smem[];
  ench8* frag = reinterpret_cast<ench8*>(simf_smem);   // [AT][T][2][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int T = a.T, d = a.d;
  const int tile0 = blockIdx.y * AT;
  const int nt = a.tiles - tile0 < AT ? a.tiles - tile0 : AT;   // tiles of this workgroup (>= 1)
  {
    const ench8* src = a.img + (size_t)tile0 * T * 128;
    for (int i = tid; i < nt * T * 128; i += SIMF_WAVES * 64) frag[i] = src[i];
  }
  const int ea = a.head->ea, eb = ea - 1;
  const float amaxn = a.head->amaxn;
  const float sc = __builtin_ldexpf(1.0f, eb), us = __builtin_ldexpf(1.0f, -(ea + eb));   // (|ea|, |eb|, |ea + eb| <= ENC_MAX_EXP + 1: normal numbers)
  const float am_max = __builtin_ldexpf(1.0f, 15 - eb), bn_min = __builtin_ldexpf(1.0f, -(eb + 3));
  const float INF = __builtin_huge_valf();
  constexpr bool vec4 = VEC4;   // d % 4 == 0 (a template parameter: the scalar loads' addresses would cost the other path its registers)
  __syncthreads();
  for (int strip = blockIdx.x * SIMF_WAVES + wave; strip < a.W; strip += gridDim.x * SIMF_WAVES) {
    const int j = strip * 32 + r;
    const int32_t row = j < a.nb ? a.b_rows[j] : -1;
    const float* x = a.rows + (size_t)(row >= 0 ? row : 0) * d;
    const bool live = row >= 0;
    encacc acc[AT];
#pragma unroll
    for (int k = 0; k < AT; ++k)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[k][v] = 0.0f;
    float pf[SIMF_PF][8];
#pragma unroll
    for (int u = 0; u < SIMF_PF; ++u) simf_load8(x, 16 * u + 8 * h, d, live, vec4, pf[u]);
    float n2 = 0.0f, am = 0.0f;
    for (int t0 = 0; t0 < T; t0 += SIMF_PF) {
#pragma unroll
      for (int u = 0; u < SIMF_PF; ++u) {
        const int t = t0 + u;
        if (t < T) {   // (uniform)
          float v[8];
#pragma unroll
          for (int w = 0; w < 8; ++w) v[w] = pf[u][w];
          if (t + SIMF_PF < T) simf_load8(x, 16 * (t + SIMF_PF) + 8 * h, d, live, vec4, pf[u]);
#pragma unroll
          for (int w = 0; w < 8; ++w) { n2 = __builtin_fmaf(v[w], v[w], n2); am = fmaxf(am, __builtin_fabsf(v[w])); }
          ench8 bh, bl;
          asf_split8(v, sc, bh, bl);
#pragma unroll
          for (int k = 0; k < AT; ++k) {
            if (k < nt) {
              const ench8 ah = frag[((size_t)(k * T + t) * 2 + 0) * 64 + lane], al = frag[((size_t)(k * T + t) * 2 + 1) * 64 + lane];
              acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[k], 0, 0, 0);
              acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[k], 0, 0, 0);
              acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[k], 0, 0, 0);
            }
          }
        }
      }
    }
    n2 += __shfl_xor(n2, 32, 64);
    am = fmaxf(am, __shfl_xor(am, 32, 64));
    const float root = __builtin_sqrtf(n2);
    const float bn = root * (1.0f + 2e-5f) + 0x1p-69f;
    const float eps = a.eps_rel * (bn * amaxn) + ENC_EPS_ABS;
    const bool b_known = row >= 0;
    const bool b_fit = n2 < INF && eps < 1e30f && am <= am_max && (root >= bn_min || am == 0.0f);   // (false for NaN)
    if (a.b_eps && blockIdx.y == 0 && h == 0 && j < a.nb) { a.b_eps[j] = eps; a.b_fit[j] = b_fit ? 1 : 0; }
    const uint32_t b_known32 = (uint32_t)__ballot(b_known), b_unfit32 = (uint32_t)__ballot(!b_fit);   // (the halves of the wave hold the same 32 columns)
#pragma unroll
    for (int k = 0; k < AT; ++k) {
      if (k < nt) {
        const int tile = tile0 + k;
        // the ballot of register v: its low half is result row 8 (v / 4) + v % 4 x the strip's 32 B rows, its high half the row four
        // below; the lane of either row keeps it, so that lane r ends up with the word of row r.  (ln is the lane number made opaque: the
        // 32 compares of a tile are loop invariants, and hoisted out of the strip loop they are 64 scalar registers per tile -- spills.)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t word = 0;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int bit = 8 * (v >> 2) + (v & 3);
          const unsigned long long m = __ballot(__builtin_fmaf(acc[k][v], us, eps) >= a.threshold);
          word = ln == bit ? (uint32_t)m : word;
          word = ln == bit + 4 ? (uint32_t)(m >> 32) : word;
        }
        // the rows' and the columns' own bits, a word at a time: an unfit row or column makes every known pair a candidate
        const bool a_known = ((a.amask[2 * tile] >> (ln & 31)) & 1u) != 0u, a_unfit = ((a.amask[2 * tile + 1] >> (ln & 31)) & 1u) != 0u;
        word = a_unfit ? 0xffffffffu : (word | b_unfit32);
        word = a_known ? (word & b_known32) : 0u;
        if (lane < 32) a.bitmap[(size_t)(tile * 32 + lane) * a.W + strip] = word;
        if (a.all_a && j < a.nb) {   // (all_a has tiles * 32 rows)
#pragma unroll
          for (int v = 0; v < 16; ++v) a.all_a[(size_t)(tile * 32 + 8 * (v >> 2) + 4 * h + (v & 3)) * a.nb + j] = acc[k][v] * us;
        }
      }
    }
  }
}

// cnt[u] = popcount(words[u]) and part[c] = the sum over chunk c of SIM_CHUNK words: what sim_scan_kernel reads.  Over the bitmap
// (row-major: i ascending, then j ascending) and over the refine's 0 / 1 flags.
static __global__ __launch_bounds__(256) void simf_count_kernel(const uint32_t* __restrict__ words, int64_t n, int32_t* __restrict__ cnt,
                                                                int32_t* __restrict__ part) {
  __shared__ int32_t wave_sum[4];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * SIM_CHUNK + 4 * tid;
  int32_t c[4];
  if (i0 + 4 <= n) {
    const uint4 w = *reinterpret_cast<const uint4*>(words + i0);
    c[0] = __popc(w.x); c[1] = __popc(w.y); c[2] = __popc(w.z); c[3] = __popc(w.w);
    int4 o; o.x = c[0]; o.y = c[1]; o.z = c[2]; o.w = c[3];
    *reinterpret_cast<int4*>(cnt + i0) = o;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[k] = i0 + k < n ? __popc(words[i0 + k]) : 0;
      if (i0 + k < n) cnt[i0 + k] = c[k];
    }
  }
  int32_t s = c[0] + c[1] + c[2] + c[3];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// the set bits of word u = (row u / W, strip u % W) at off[u] .., ascending
static __global__ __launch_bounds__(256) void simf_list_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ off, int64_t n, int W,
                                                               int32_t* __restrict__ ci, int32_t* __restrict__ cj) {
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n; u += (int64_t)gridDim.x * 256) {
    uint32_t w = words[u];
    if (!w) continue;
    const int i = (int)(u / W), j0 = (int)(u - (int64_t)i * W) * 32;
    int32_t p = off[u];
    while (w) {
      ci[p] = i;
      cj[p] = j0 + __ffs(w) - 1;
      ++p;
      w &= w - 1;
    }
  }
}

struct SimfRefineArgs {
  const int32_t* ci;        // [n] A row of the pass
  const int32_t* cj;        // [n] position in the B argument
  const int32_t* b_rows;    // [nb]
  const float* a;           // [rows of the pass][d]
  const float* rows;        // [N][d]
  float* sim;               // [n] the chain
  uint32_t* flag;           // [n] 1: sim_float4gt(chain, threshold)
  int n, d;
  float threshold;
};

static __global__ __launch_bounds__(64) void simf_refine_kernel(SimfRefineArgs a) {
  __shared__ __attribute__((aligned(16))) float ta[TILE_FLOATS];   // [TILE_DCH][TILE_STRIDE] A rows
  __shared__ __attribute__((aligned(16))) float tb[TILE_FLOATS];   // B rows
  const int lane = threadIdx.x, d = a.d;
  const int c = blockIdx.x * 64 + lane;
  const int32_t ra = c < a.n ? a.ci[c] : -1;
  const int32_t rb = c < a.n ? a.b_rows[a.cj[c]] : -1;   // (a candidate's rows are known)
  float acc = 0.0f;
  const bool vec4 = (d & 3) == 0;
  for (int c0 = 0; c0 < d; c0 += TILE_DCH) {
    const int nd = (d - c0 < TILE_DCH) ? d - c0 : TILE_DCH;
    float4 va[8], vb[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      va[it] = tile_row_piece(a.a, ra, it, lane, d, c0, nd, vec4);
      vb[it] = tile_row_piece(a.rows, rb, it, lane, d, c0, nd, vec4);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      tile_store_row_piece(ta, va[it], it, lane);
      tile_store_row_piece(tb, vb[it], it, lane);
    }
    wave_lds_sync();
    chain1<TILE_STRIDE, TILE_STRIDE>(acc, ta + lane, tb + lane, nd);   // v1: the A row
    wave_lds_sync();
  }
  if (c < a.n) {
    a.sim[c] = acc;
    a.flag[c] = sim_float4gt(acc, a.threshold) ? 1u : 0u;
  }
}

// the matching candidates at their scanned rank, the first `cap` of them (sim_fill_kernel's rule)
static __global__ __launch_bounds__(256) void simf_out_kernel(const int32_t* __restrict__ ci, const int32_t* __restrict__ cj, const float* __restrict__ sim,
                                                              const uint32_t* __restrict__ flag, const int32_t* __restrict__ off, int n, int a0, int32_t cap,
                                                              int32_t* __restrict__ out_a, int32_t* __restrict__ out_b, float* __restrict__ out_sim) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n || !flag[c]) return;
  const int32_t p = off[c];
  if (p < cap) { out_a[p] = a0 + ci[c]; out_b[p] = cj[c]; out_sim[p] = sim[c]; }
}

// check_brackets bit 5: every known fit pair of the pass against the chain sim_matrix_kernel wrote; viol[0] += violated, [1] += checked
static __global__ __launch_bounds__(256) void simf_check_kernel(const float* __restrict__ all_a, const float* __restrict__ blk, const float* __restrict__ b_eps,
                                                                const uint8_t* __restrict__ b_fit, const uint8_t* __restrict__ known_b,
                                                                const uint32_t* __restrict__ amask, int n, int nb, int32_t* viol) {
  int chk = 0, bad = 0;
  const int64_t total = (int64_t)n * nb;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int i = (int)(p / nb), j = (int)(p - (int64_t)i * nb);
    const bool a_fit = ((amask[2 * (i >> 5)] >> (i & 31)) & 1u) != 0u && ((amask[2 * (i >> 5) + 1] >> (i & 31)) & 1u) == 0u;
    if (!a_fit || !known_b[j] || !b_fit[j]) continue;
    ++chk;
    if (!(__builtin_fabsf(all_a[p] - blk[p]) <= b_eps[j])) ++bad;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { chk += __shfl_xor(chk, o, 64); bad += __shfl_xor(bad, o, 64); }
  if ((threadIdx.x & 63) == 0) {
    if (chk) atomicAdd(viol + 1, chk);
    if (bad) atomicAdd(viol + 0, bad);
  }
}

}  // namespace freddy
