// analogy.h -- exact word analogies: analogy_3cosadd / analogy_3cosadd_in / analogy_3cosmul
// (freddy--0.0.1.sql:1270-1315, 1231-1249), the functions analogy(a, b, c) / analogy_in(...) dispatch to by default
// (:198-199, :269-297), and analogy_pair_direction (:1212-1229; its contract further down).
//
// Contract.  Inputs are rows w1, w2, w3 of the table (v1, v2, v3); v4 runs over the candidate rows.  cos(a, b) is
// cosine_similarity_bytea (core_functions.c:67-81): the binary32 chain "s += a[i] * b[i]", i ascending, multiply and add
// each rounded -- exact.h's arithmetic, bit for bit.
//   3CosAdd  raw = (v3 - v1) + v2 elementwise in binary32 (vec_minus_bytea / vec_plus_bytea, core_functions.c:120-196);
//            score = cos(raw, v4), a binary32 value (reported widened to double).
//   3CosMul  score = ((c3 + 1)/2) * ((c2 + 1.0)/2.0) / (((c1 + 1.0)/2.0) + 0.001) with c_i = cos(v4, v_i).  PostgreSQL
//            resolves float4 + int and float4 + numeric to float48pl (float8 is the preferred type), so the whole expression
//            is FLOAT8: every c_i widened to double, the constants are the doubles nearest 1, 2 and 0.001, evaluated as
//            (A * B) / D.  No PostgreSQL confirms this reading here: an_mul_score below and the test model
//            (tests/analogy_model.py: mul_score) are the ONE place to change if it is shown otherwise.
//   Both:    rows whose id is w1, w2 or w3 are excluded (WHERE v4.word NOT IN (...)); a different row with an identical vector
//            is not.  Order: score DESC, then id ASC (the pinned tie-break, as exact.h; PostgreSQL leaves it unspecified).
//            FETCH FIRST 1 -> the first k.  NaN scores sort first (PostgreSQL's float8 order); -0 and +0 are one value (the
//            score of a -0 is reported as +0).  PostgreSQL's float8 overflow / division-by-zero errors cannot arise for a
//            finite normalised table; here such a row simply scores inf / NaN.  An unknown input id: the INNER JOIN is empty,
//            every slot of that analogy is (-1, -inf) (the host resolves ids, no device work).
//
// Two paths (analogy.hip: freddy_gpu_exact_analogy -> analogy_scan / analogy_filter; what the filter shares with exact kNN: exact_host.h):
//
// ALL-EXACT (an_scan_kernel + an_merge_kernel): every eligible row's score from the reference's chains -- one query column
//   per analogy for 3CosAdd, three for 3CosMul -- in exact_scan_kernel's style (64-row blocks, lane = row, columns in LDS).
//   For "id = ANY(set)" subsets, tables below 8192 rows or not finite, exact_filter = 0, and 3CosMul on tables wider than
//   416 dimensions (its three tiles of query fragments would not fit a CU's 160 KiB of LDS: an_filter_lds).
//
// FILTER + REFINE over the whole table (exact2.h's machinery, the same eligibility as exact kNN):
//   * The pass: up to 32 analogies.  3CosMul puts v1, v2, v3 of analogy j into column j of three 32-column B tiles, so one lane
//     holds all three approximate cosines a_1..a_3 of its rows for one analogy and the epilogue needs no cross-lane traffic (96
//     columns per pass of the table); 3CosAdd has one tile (raw).  exf_prep_kernel builds the fragments, exf_strip_mfma runs
//     the table's fragment copy (exf_layout_kernel: no new HBM copy) against them.
//   * Bracket: the reference's c_i lies in [a_i - eps_i, a_i + eps_i], eps_i = EXF_EPS X |v_i| (exact2.h:25-31).
//   * Score bounds [lo, hi] (an_bounds_*).  Proof sketch.  Let L_i <= c_i <= H_i (doubles: a_i -/+ eps_i, rounded outward).
//     Every step of the reference's float8 evaluation is a correctly rounded IEEE operation, and rounding is monotone: if
//     x <= y then fl(x) <= fl(y).  So t_i = fl(fl(c_i + 1) / 2) lies in [fl(fl(L_i + 1)/2), fl(fl(H_i + 1)/2)], and D =
//     fl(t_1 + 0.001) likewise.  The real product A B over the box [A] x [B] takes its extremes at the corners; fl of it lies
//     between fl of the smallest and fl of the largest corner product (monotone again) -- whatever the signs (the table need
//     not be normalised).  For D > 0 the real quotient P / D over the box takes its maximum at Ph / Dl if Ph >= 0 else Ph / Dh
//     and its minimum at Pl / Dh if Pl >= 0 else Pl / Dl, and fl of it is bracketed by fl of those.  Evaluating the same
//     expression, in the same order, on the interval ends therefore bounds the reference's double score EXACTLY: no widening
//     beyond the first step.  If the D interval is not strictly positive, lo = -inf and hi = +inf (always a candidate).
//     3CosAdd: [L, H] itself (the float score is exactly representable in double).
//   * Threshold: tau = the k-th largest lo among the sample rows (EXF_SAMPLE rows, whole strips spread over the table) with the
//     analogy's three input rows EXCLUDED -- an input row is usually the best row of all (v3 has c3 ~ 1) and would set tau above
//     the true answer.  At least k non-input sample rows have score >= lo >= tau, so the k-th best score S_k >= tau.
//   * Candidates: non-input rows with hi >= tau: every row of the answer has hi >= score >= S_k >= tau (ties included).  A pass
//     whose candidate buffer overflows (or whose columns are not finite) is redone on the all-exact path: nothing is dropped.
//   * Refine: the reference's chains from the row-major copy (exact.h's arithmetic), the double combination, the selection.
//     check_brackets bit 3 makes every row a candidate (inputs included, for the check only) and counts rows with a c_i
//     outside its bracket in freddy_gpu_filter_bound_violations / _checked.
//
// PAIR DIRECTION (analogy_pair_direction, freddy--0.0.1.sql:1212-1229; method FREDDY_ANALOGY_PAIR_DIRECTION).  The one search
// function of the reference that scans the ORIGINAL (un-normalised) table, get_vecs_name_original(); the device does not care
// which table the handle holds.  For rows w1, w2, w3 and every candidate row v4 whose id is none of the three inputs:
//   A  = vec_normalize_bytea(vec_minus_bytea(v1, v2))      once per analogy
//   U4 = vec_normalize_bytea(vec_minus_bytea(v3, v4))      per candidate row
//   score = cosine_similarity_bytea(A, U4)                  a binary32 value (reported widened to double, as 3CosAdd's)
//   ORDER BY score DESC, FETCH FIRST 1 (here: the first k; ties by id ASC, the pinned tie-break).
// All arithmetic is binary32, operation by operation, as core_functions.c does it (no contraction: -ffp-contract=off):
//   vec_minus_bytea (:120-139)      t[i] = a[i] - b[i]
//   vec_normalize_bytea (:243-269)  sq += t[i] * t[i], i ascending, multiply and add each rounded; length = (float)sqrt((double)sq);
//                                   out[i] = t[i] / length, a correctly rounded binary32 division (the v_div_scale / v_div_fmas /
//                                   v_div_fixup sequence with fp32 denormals on -- never a reciprocal multiply).  The kernels
//                                   take the square root in the reference's own form, the double square root rounded to float
//                                   (equal to the correctly rounded float square root for every float: 53 >= 2 * 24 + 2 bits);
//                                   it runs once per (row, analogy) against d divisions, so its cost does not show.
//   cosine_similarity_bytea         s += A[i] * U4[i], i ascending: exact.h's chain.
// What follows from that, none of it special-cased:
//   * a row with v3's vector under another id has length 0, every component of U4 is 0/0, its score is NaN, and NaN sorts FIRST
//     (an_ord): such a duplicate wins;
//   * w1 == w2 (or equal vectors) makes A all NaN and every score NaN: the answer is the k lowest ids that are not inputs;
//   * -0 and +0 are one value, reported as +0; an unknown input id gives (-1, -inf) in every slot with no device work;
//   * non-finite tables need no other path: there is no filter, the arithmetic just runs.
// The score is not a dot product against a fixed query column (the candidate row is normalised per (analogy, row) before the
// chain), so neither the MFMA filter nor an_scan_kernel's accumulate loop expresses it: an_pair_columns_kernel writes A and a copy
// of v3 per analogy, an_pair_scan_kernel makes two sweeps over a row's dimensions (the sums of squares of v3 - x, then the
// chain with the difference recomputed -- the same rounded value), an_merge_kernel merges as for the other methods.  There is
// no filter + refine path: an MFMA bound on A . (v3 - v4) / |v3 - v4| loses its grip exactly where rows are close to v3;
// exact_filter and check_brackets have no effect on this method.
//
// Selection key: (score DESC, row ASC) does not fit exact.h's u64 (float, row) key for a double score, and the double is not
// rounded to a float: an_ord maps the double to an order-preserving u64, and the selection (AnTop) compares (ord, row) pairs
// -- a wave's k <= 32 best in LDS, arrivals that beat the k-th merged in by rank.
//
// Roofline (3 M x 300, one pass of 32 analogies): the fragment copy streams once, 3.6 GB = 0.6-0.7 ms at 5.1-6.1 TB/s; MFMA
// work 3 x 2 N d 96 = 0.5 PFLOP-equivalents ~ 0.25 ms at ~2 PF/s, below the HBM time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dot_chain.h"
#include "exact.h"
#include "exact2.h"
#include "wave_topk.h"

namespace freddy {

static constexpr int AN_MAXK = 32;         // k limit of the exact analogy
static constexpr int AN_PASS = 32;         // analogies per filter pass (one column of each tile)
static constexpr int AN_WG = 256;          // all-exact scan / merge / threshold: four waves
static constexpr int AN_WAVES = AN_WG / 64;
static constexpr int AN_RW = 8;            // waves of a refine workgroup (one analogy)
static constexpr int AN_SLOTS = AN_MAXK + 64;   // a wave's list and the arrivals behind it
static constexpr uint32_t AN_NO_ROW = 0xffffffffu;
static constexpr size_t AN_MAX_LDS = 160 * 1024;   // dynamic LDS a workgroup may ask for (a gfx950 CU has 160 KiB)

// an_filter_kernel's LDS: the pass's M tiles of query fragments.  3CosMul (M = 3) fits for d <= 416 (T <= 26); wider tables
// answer 3CosMul on the all-exact path
static inline size_t an_filter_lds(int M, int d) { return (size_t)M * ((d + 15) / 16) * 2 * 64 * 16; }

struct AnEnt { u64 ord; uint32_t row; uint32_t pad; };   // a partial list entry (row AN_NO_ROW: empty)

// order-preserving map of a double (NaN above everything, -0 == +0); 0 is no score's image (the empty entry)
__device__ __forceinline__ u64 an_ord(double s) {
  if (s != s) return ~0ull;
  s = s + 0.0;
  const u64 b = (u64)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double an_unord(u64 o) {
  if (o == ~0ull) return __longlong_as_double(0x7ff8000000000000ll);
  const u64 b = (o >> 63) ? (o & 0x7fffffffffffffffull) : ~o;
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ bool an_better(u64 oa, uint32_t ra, u64 ob, uint32_t rb) { return oa > ob || (oa == ob && ra < rb); }

// The reference's 3CosMul expression (freddy--0.0.1.sql:1243) in float8; c_i = cos(v4, v_i)
__device__ __forceinline__ double an_mul_score(float c1, float c2, float c3) {
  const double A = ((double)c3 + 1.0) / 2.0;
  const double B = ((double)c2 + 1.0) / 2.0;
  const double D = ((double)c1 + 1.0) / 2.0 + 0.001;
  return (A * B) / D;
}

// [a - e, a + e] as doubles, rounded outward (the one step whose exactness is not given: a double difference of two floats
// far apart in magnitude may round)
__device__ __forceinline__ void an_bracket(float a, float e, double& L, double& H) {
  const double l = (double)a - (double)e, h = (double)a + (double)e;
  L = l - __builtin_fabs(l) * 0x1p-52 - 0x1p-1000;
  H = h + __builtin_fabs(h) * 0x1p-52 + 0x1p-1000;
}
__device__ __forceinline__ void an_bounds_add(float a, float e, double& lo, double& hi) { an_bracket(a, e, lo, hi); }
__device__ __forceinline__ void an_bounds_mul(const float (&a)[3], const float (&e)[3], double& lo, double& hi) {
  double L[3], H[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) an_bracket(a[n], e[n], L[n], H[n]);
  const double Al = (L[2] + 1.0) / 2.0, Ah = (H[2] + 1.0) / 2.0;
  const double Bl = (L[1] + 1.0) / 2.0, Bh = (H[1] + 1.0) / 2.0;
  const double Dl = (L[0] + 1.0) / 2.0 + 0.001, Dh = (H[0] + 1.0) / 2.0 + 0.001;
  if (!(Dl > 0.0)) { lo = -__builtin_huge_val(); hi = __builtin_huge_val(); return; }
  const double p0 = Al * Bl, p1 = Al * Bh, p2 = Ah * Bl, p3 = Ah * Bh;
  const double Pl = fmin(fmin(p0, p1), fmin(p2, p3)), Ph = fmax(fmax(p0, p1), fmax(p2, p3));
  hi = Ph >= 0.0 ? Ph / Dl : Ph / Dh;
  lo = Pl >= 0.0 ? Pl / Dh : Pl / Dl;
}

// A wave's k best (ord, row) pairs in LDS, best first, with room for 64 arrivals behind them.  push() is called by all 64
// lanes with wave-uniform control flow; keys are distinct (a row arrives once per list).
struct AnTop {
  u64* ord; uint32_t* row;   // [AN_SLOTS]
  int cnt, k;
  u64 tord; uint32_t trow;   // the k-th entry once cnt == k
  __device__ void init(u64* o, uint32_t* r, int k_) { ord = o; row = r; cnt = 0; k = k_; tord = 0; trow = AN_NO_ROW; }
  __device__ void push(u64 o, uint32_t r, bool valid) {
    const int lane = threadIdx.x & 63;
    const bool take = valid && (cnt < k || an_better(o, r, tord, trow));
    const u64 m = __ballot(take);
    if (m == 0ull) return;
    if (take) {
      const int p = cnt + __popcll(m & ((1ull << lane) - 1ull));
      ord[p] = o; row[p] = r;
    }
    const int total = cnt + __popcll(m);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    u64 eo[2]; uint32_t er[2]; int rk[2] = {AN_SLOTS, AN_SLOTS};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < total) {
        eo[h] = ord[i]; er[h] = row[i];
        int c = 0;
        for (int j = 0; j < total; ++j) c += an_better(ord[j], row[j], eo[h], er[h]) ? 1 : 0;
        rk[h] = c;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (rk[h] < k) { ord[rk[h]] = eo[h]; row[rk[h]] = er[h]; }
    cnt = total < k ? total : k;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (cnt == k) { tord = ord[k - 1]; trow = row[k - 1]; }
  }
};

// The lists of W waves (lists at ords + w * AN_SLOTS, counts in cnts[w]) into wave 0's; called by wave 0 after a barrier.
__device__ __forceinline__ void an_absorb(AnTop& top, const u64* ords, const uint32_t* rows, const int* cnts, int W) {
  const int lane = threadIdx.x & 63;
  for (int w = 1; w < W; w += 2) {   // two lists per push: lanes 0..31 and 32..63
    const int ww = w + (lane >> 5), i = lane & 31;
    const bool v = ww < W && i < cnts[ww < W ? ww : 0];
    const u64 o = v ? ords[ww * AN_SLOTS + i] : 0ull;
    const uint32_t r = v ? rows[ww * AN_SLOTS + i] : AN_NO_ROW;
    top.push(o, r, v);
  }
}

// ---- the analogies' query columns --------------------------------------------------------------------------------
// in_rows[a][3] = table rows of w1, w2, w3.  M = 1 (3CosAdd): raw = (v3 - v1) + v2; M = 3 (3CosMul): v1, v2, v3.
// PASS layout (filter path): column m * 32 + j for analogy a0 + j (zero for j >= na), as exf_prep_kernel wants the tiles;
// otherwise column a * M + m (a < na).  One workgroup per column.
__global__ __launch_bounds__(256) void an_gather_kernel(const float* __restrict__ rows, int d, const int32_t* __restrict__ in_rows,
                                                       int na, int M, int pass_layout, float* __restrict__ out) {
  const int c = blockIdx.x;
  int a, m;
  if (pass_layout) { m = c / AN_PASS; a = c - m * AN_PASS; }
  else { a = c / M; m = c - a * M; }
  float* o = out + (size_t)c * d;
  if (a >= na) { for (int i = threadIdx.x; i < d; i += 256) o[i] = 0.0f; return; }
  const int32_t* r = in_rows + (size_t)a * 3;
  if (M == 1) {
    const float *v1 = rows + (size_t)r[0] * d, *v2 = rows + (size_t)r[1] * d, *v3 = rows + (size_t)r[2] * d;
    for (int i = threadIdx.x; i < d; i += 256) { const float t = v3[i] - v1[i]; o[i] = t + v2[i]; }   // vec_plus(vec_minus(v3, v1), v2)
  } else {
    const float* v = rows + (size_t)r[m] * d;
    for (int i = threadIdx.x; i < d; i += 256) o[i] = v[i];
  }
}

// ---- all-exact path ------------------------------------------------------------------------------------------------
struct AnScanArgs {
  const float* xb;          // [blocks][d][64]
  const int32_t* pos;       // [blocks*64] table row of each slot (-1 padding) or NULL: the slot is the row, below n_rows
  int64_t n_rows;
  int n_blocks, chunk_blocks, nchunk;
  const float* cols;        // [na * M][d]
  const int32_t* in_rows;   // [na][3]
  int na, d, k;
  AnEnt* part;              // [na][nchunk * AN_WAVES][k]
};
template <int M, int AT>
__global__ __launch_bounds__(AN_WG) void an_scan_kernel(AnScanArgs a) {
  constexpr int QC = M * AT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);                                                    // [d][QC]
  u64* lo = reinterpret_cast<u64*>(smem + (((size_t)a.d * QC * 4 + 15) & ~(size_t)15));          // [waves][AT][AN_SLOTS]
  uint32_t* lr = reinterpret_cast<uint32_t*>(lo + AN_WAVES * AT * AN_SLOTS);
  const int chunk = blockIdx.x, a0 = blockIdx.y * AT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, d = a.d;
  for (int i = threadIdx.x; i < d * QC; i += AN_WG) {
    const int c = i / d, dim = i - c * d;
    const int an = (a0 + c / M < a.na) ? a0 + c / M : a.na - 1;
    qs[dim * QC + c] = a.cols[((size_t)an * M + c % M) * d + dim];
  }
  int32_t ex[AT][3];
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int m = 0; m < 3; ++m) ex[t][m] = (a0 + t < a.na) ? a.in_rows[(size_t)(a0 + t) * 3 + m] : -2;
  __syncthreads();
  AnTop top[AT];
#pragma unroll
  for (int t = 0; t < AT; ++t) top[t].init(lo + ((size_t)wave * AT + t) * AN_SLOTS, lr + ((size_t)wave * AT + t) * AN_SLOTS, a.k);
  const int b0 = chunk * a.chunk_blocks;
  const int b1 = (b0 + a.chunk_blocks < a.n_blocks) ? b0 + a.chunk_blocks : a.n_blocks;
  for (int b = b0 + wave; b < b1; b += AN_WAVES) {
    const float* xrow = a.xb + (size_t)b * d * 64 + lane;
    float acc[QC];
#pragma unroll
    for (int c = 0; c < QC; ++c) acc[c] = 0.0f;
    // (dot_chain.h's stream_row, kept in place for registers: profiles/HISTORY.md, the dot_chain.h entry)
    constexpr int DB = 8;
    float xn[DB];
#pragma unroll
    for (int u = 0; u < DB; ++u) xn[u] = (u < d) ? xrow[(size_t)u * 64] : 0.0f;
    for (int i0 = 0; i0 < d; i0 += DB) {
      float xc[DB];
#pragma unroll
      for (int u = 0; u < DB; ++u) xc[u] = xn[u];
#pragma unroll
      for (int u = 0; u < DB; ++u) xn[u] = (i0 + DB + u < d) ? xrow[(size_t)(i0 + DB + u) * 64] : 0.0f;
#pragma unroll
      for (int u = 0; u < DB; ++u) {
        const int i = i0 + u;
        if (i < d) {
          const float* q = qs + i * QC;
#pragma unroll
          for (int c = 0; c < QC; ++c) { const float p = q[c] * xc[u]; acc[c] = acc[c] + p; }   // core_functions.c:77
        }
      }
    }
    const int64_t slot = (int64_t)b * 64 + lane;
    const int32_t row = a.pos ? a.pos[slot] : (slot < a.n_rows ? (int32_t)slot : -1);
#pragma unroll
    for (int t = 0; t < AT; ++t) {
      const double s = (M == 1) ? (double)acc[t] : an_mul_score(acc[t * M + 0], acc[t * M + 1], acc[t * M + 2]);
      const bool ok = row >= 0 && a0 + t < a.na && row != ex[t][0] && row != ex[t][1] && row != ex[t][2];
      top[t].push(an_ord(s), (uint32_t)row, ok);
    }
  }
#pragma unroll
  for (int t = 0; t < AT; ++t) {
    if (a0 + t >= a.na) continue;
    AnEnt* out = a.part + (((size_t)(a0 + t) * a.nchunk + chunk) * AN_WAVES + wave) * a.k;
    for (int r = lane; r < a.k; r += 64) {
      const bool v = r < top[t].cnt;
      out[r] = AnEnt{v ? top[t].ord[r] : 0ull, v ? top[t].row[r] : AN_NO_ROW, 0u};
    }
  }
}

// ---- pair direction ------------------------------------------------------------------------------------------------------
// The columns of the pair-direction scan, one workgroup (one wave) per analogy: out[a][0][d] = A = vec_normalize(v1 - v2),
// out[a][1][d] = v3.  The sum of squares is the reference's sequential chain: one lane walks it.
__global__ __launch_bounds__(64) void an_pair_columns_kernel(const float* __restrict__ rows, int d, const int32_t* __restrict__ in_rows,
                                                            float* __restrict__ out) {
  __shared__ float len_s;
  const int a = blockIdx.x, lane = threadIdx.x;
  const int32_t* r = in_rows + (size_t)a * 3;
  const float *v1 = rows + (size_t)r[0] * d, *v2 = rows + (size_t)r[1] * d, *v3 = rows + (size_t)r[2] * d;
  float* A = out + (size_t)a * 2 * d;
  for (int i = lane; i < d; i += 64) { A[i] = v1[i] - v2[i]; A[d + i] = v3[i]; }   // vec_minus_bytea(v1, v2)
  __syncthreads();
  if (lane == 0) {
    float sq = 0.0f;
    for (int i = 0; i < d; ++i) { const float p = A[i] * A[i]; sq = sq + p; }       // core_functions.c:255-257
    len_s = (float)sqrt((double)sq);
  }
  __syncthreads();
  const float len = len_s;
  for (int i = lane; i < d; i += 64) A[i] = A[i] / len;
}

// The pair-direction scan: an_scan_kernel's layout (64-row blocks, lane = row, AT analogies per workgroup, one AnTop per (wave,
// analogy), partial lists for an_merge_kernel) around two sweeps over the row's dimensions.  a.cols = an_pair_columns_kernel's
// output; in LDS dimension i holds [A_0 .. A_AT-1, v3_0 .. v3_AT-1].
template <int AT>
__global__ __launch_bounds__(AN_WG) void an_pair_scan_kernel(AnScanArgs a) {
  constexpr int QC = 2 * AT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);                                                    // [d][QC]
  u64* lo = reinterpret_cast<u64*>(smem + (((size_t)a.d * QC * 4 + 15) & ~(size_t)15));          // [waves][AT][AN_SLOTS]
  uint32_t* lr = reinterpret_cast<uint32_t*>(lo + AN_WAVES * AT * AN_SLOTS);
  const int chunk = blockIdx.x, a0 = blockIdx.y * AT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, d = a.d;
  for (int i = threadIdx.x; i < d * QC; i += AN_WG) {
    const int c = i / d, dim = i - c * d;        // c = h * AT + t: h = 0 the A column, 1 the v3 column of analogy a0 + t
    const int h = c / AT, t = c - h * AT;
    const int an = (a0 + t < a.na) ? a0 + t : a.na - 1;
    qs[dim * QC + c] = a.cols[((size_t)an * 2 + h) * d + dim];
  }
  int32_t ex[AT][3];
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int m = 0; m < 3; ++m) ex[t][m] = (a0 + t < a.na) ? a.in_rows[(size_t)(a0 + t) * 3 + m] : -2;
  __syncthreads();
  AnTop top[AT];
#pragma unroll
  for (int t = 0; t < AT; ++t) top[t].init(lo + ((size_t)wave * AT + t) * AN_SLOTS, lr + ((size_t)wave * AT + t) * AN_SLOTS, a.k);
  const int b0 = chunk * a.chunk_blocks;
  const int b1 = (b0 + a.chunk_blocks < a.n_blocks) ? b0 + a.chunk_blocks : a.n_blocks;
  for (int b = b0 + wave; b < b1; b += AN_WAVES) {
    const float* xrow = a.xb + (size_t)b * d * 64 + lane;
    float sq[AT], len[AT], acc[AT];
#pragma unroll
    for (int t = 0; t < AT; ++t) { sq[t] = 0.0f; acc[t] = 0.0f; }
    stream_row(xrow, d, [&](int i, float x) {            // sweep 1: vec_normalize_bytea's sum of squares of v3 - v4
      const float* q = qs + i * QC + AT;
#pragma unroll
      for (int t = 0; t < AT; ++t) { const float df = q[t] - x; const float p = df * df; sq[t] = sq[t] + p; }
    });
#pragma unroll
    for (int t = 0; t < AT; ++t) len[t] = (float)sqrt((double)sq[t]);                            // core_functions.c:259
    stream_row(xrow, d, [&](int i, float x) {            // sweep 2: the cosine chain over A and (v3 - v4) / length
      const float* q = qs + i * QC;
#pragma unroll
      for (int t = 0; t < AT; ++t) {
        const float df = q[AT + t] - x;                     // (recomputed: the same rounded value as in sweep 1)
        const float u = df / len[t];
        const float p = q[t] * u;
        acc[t] = acc[t] + p;
      }
    });
    const int64_t slot = (int64_t)b * 64 + lane;
    const int32_t row = a.pos ? a.pos[slot] : (slot < a.n_rows ? (int32_t)slot : -1);
#pragma unroll
    for (int t = 0; t < AT; ++t) {
      const bool ok = row >= 0 && a0 + t < a.na && row != ex[t][0] && row != ex[t][1] && row != ex[t][2];
      top[t].push(an_ord((double)acc[t]), (uint32_t)row, ok);
    }
  }
#pragma unroll
  for (int t = 0; t < AT; ++t) {
    if (a0 + t >= a.na) continue;
    AnEnt* out = a.part + (((size_t)(a0 + t) * a.nchunk + chunk) * AN_WAVES + wave) * a.k;
    for (int r = lane; r < a.k; r += 64) {
      const bool v = r < top[t].cnt;
      out[r] = AnEnt{v ? top[t].ord[r] : 0ull, v ? top[t].row[r] : AN_NO_ROW, 0u};
    }
  }
}

// One workgroup per analogy: the partial lists -> the analogy's k best, (id, score) in order, (-1, -inf) beyond the rows.
__global__ __launch_bounds__(AN_WG) void an_merge_kernel(const AnEnt* __restrict__ part, int parts, int k, const int32_t* __restrict__ ids,
                                                        int32_t* __restrict__ out_ids, double* __restrict__ out_score) {
  __shared__ u64 lo[AN_WAVES * AN_SLOTS];
  __shared__ uint32_t lr[AN_WAVES * AN_SLOTS];
  __shared__ int cnts[AN_WAVES];
  const int q = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  AnTop top;
  top.init(lo + wave * AN_SLOTS, lr + wave * AN_SLOTS, k);
  const AnEnt* src = part + (size_t)q * parts * k;
  const long long total = (long long)parts * k;
  for (long long base = (long long)wave * 64; base < total; base += AN_WG) {
    const bool in = base + lane < total;
    const AnEnt e = in ? src[base + lane] : AnEnt{0ull, AN_NO_ROW, 0u};
    top.push(e.ord, e.row, in && e.row != AN_NO_ROW);
  }
  if (lane == 0) cnts[wave] = top.cnt;
  __syncthreads();
  if (wave != 0) return;
  an_absorb(top, lo, lr, cnts, AN_WAVES);
  for (int r = lane; r < k; r += 64) {
    const bool v = r < top.cnt;
    out_ids[(size_t)q * k + r] = v ? ids[top.row[r]] : -1;
    out_score[(size_t)q * k + r] = v ? an_unord(top.ord[r]) : -__builtin_huge_val();
  }
}

// ---- filter + refine path ------------------------------------------------------------------------------------------
struct AnFilterArgs {
  const h8v* xf;            // the table in fragment order
  int64_t n_rows;           // rows of this launch (SAMPLE: sample rows)
  int64_t strip_stride;     // SAMPLE: strip i of the launch is strip i * strip_stride of the table; 1 otherwise
  int T;
  const h8v* qfrag;         // [NT][T][2][64]
  const float* qunscale;    // [NT * 32]
  const float* qeps;        // [NT * 32]
  const int32_t* in_rows;   // [na][3] of the pass
  int na;
  double* sample_out;       // SAMPLE: [AN_PASS][n_rows] lower bounds, -inf for the analogy's input rows
  const double* thr;        // FILTER: [AN_PASS] tau
  int32_t* cand_cnt;        // [AN_PASS]
  uint4* cand;              // [AN_PASS][cap]: (row, bits of a_1, a_2, a_3)
  int cap, refine_all;
};
template <int NT, bool SAMPLE>
__global__ __launch_bounds__(EXF_WG, 1) void an_filter_kernel(AnFilterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  h8v* qf = reinterpret_cast<h8v*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T;
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.qfrag);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    const int n16 = NT * T * 2 * 64;
    for (int i = tid; i < n16; i += EXF_WG) dst[i] = src[i];
  }
  __syncthreads();
  const int j = lane & 31, g = lane >> 5;   // the lane's analogy (column j of every tile)
  const bool live = j < a.na;
  float unsc[NT], eps[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) { unsc[n] = a.qunscale[32 * n + j]; eps[n] = a.qeps[32 * n + j]; }
  const int32_t x1 = live ? a.in_rows[j * 3 + 0] : -2, x2 = live ? a.in_rows[j * 3 + 1] : -2, x3 = live ? a.in_rows[j * 3 + 2] : -2;
  const double thr = SAMPLE ? 0.0 : a.thr[j];
  const int64_t n_strips = (a.n_rows + 31) >> 5;
  for (int64_t strip = (int64_t)blockIdx.x * (EXF_WG / 64) + wave; strip < n_strips; strip += (int64_t)gridDim.x * (EXF_WG / 64)) {
    const int64_t tstrip = SAMPLE ? strip * a.strip_stride : strip;
    f16acc acc[NT];
    exf_strip_mfma<NT>(a.xf + (size_t)tstrip * T * 128 + lane, qf, T, lane, acc);
    // C layout: register v of lane l = row (v & 3) + 8 (v >> 2) + 4 (l >> 5) of the strip, column l & 31
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int within = (v & 3) + 8 * (v >> 2) + 4 * g;
      const int64_t r = strip * 32 + within;             // row of the launch
      const int64_t trow = tstrip * 32 + within;         // row of the table
      if (!live || r >= a.n_rows) continue;
      const bool input = trow == x1 || trow == x2 || trow == x3;
      float av[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) av[n] = acc[n][v] * unsc[n];
      double lo, hi;
      if constexpr (NT == 1) an_bounds_add(av[0], eps[0], lo, hi);
      else an_bounds_mul(av, eps, lo, hi);
      if constexpr (SAMPLE) {
        a.sample_out[(size_t)j * a.n_rows + r] = input ? -__builtin_huge_val() : lo;
      } else {
        if ((!input || a.refine_all) && !(hi < thr)) {   // (a NaN passes: the refine stage decides)
          const int slot = atomicAdd(a.cand_cnt + j, 1);
          if (slot < a.cap)
            a.cand[(size_t)j * a.cap + slot] = uint4{(uint32_t)trow, __float_as_uint(av[0]), NT > 1 ? __float_as_uint(av[NT > 1 ? 1 : 0]) : 0u,
                                                     NT > 2 ? __float_as_uint(av[NT > 2 ? 2 : 0]) : 0u};
        }
      }
    }
  }
}

// tau = the k-th largest lower bound of the sample (input rows already -inf); -inf when fewer than k rows or refine_all.
// One workgroup per analogy column; also zeroes the column's candidate count.
__global__ __launch_bounds__(AN_WG) void an_threshold_kernel(const double* __restrict__ sample, int n_sample, int na, int k, int refine_all,
                                                            double* __restrict__ thr, int32_t* __restrict__ cand_cnt) {
  __shared__ u64 lo[AN_WAVES * AN_SLOTS];
  __shared__ uint32_t lr[AN_WAVES * AN_SLOTS];
  __shared__ int cnts[AN_WAVES];
  const int j = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) cand_cnt[j] = 0;
  if (j >= na) { if (threadIdx.x == 0) thr[j] = __builtin_huge_val(); return; }
  AnTop top;
  top.init(lo + wave * AN_SLOTS, lr + wave * AN_SLOTS, k);
  const double* s = sample + (size_t)j * n_sample;
  for (int base = wave * 64; base < n_sample; base += AN_WG) {
    const int i = base + lane;
    const double x = i < n_sample ? s[i] : 0.0;
    top.push(an_ord(x == x ? x : -__builtin_huge_val()), (uint32_t)i, i < n_sample);
  }
  if (lane == 0) cnts[wave] = top.cnt;
  __syncthreads();
  if (wave != 0) return;
  an_absorb(top, lo, lr, cnts, AN_WAVES);
  if (lane == 0) thr[j] = (top.cnt < k || refine_all) ? -__builtin_huge_val() : an_unord(top.ord[k - 1]);
}

// One workgroup per analogy of the pass: the reference's chains for the candidates, the score, the k best.
struct AnRefineArgs {
  const float* rows;        // [N][d] row-major
  const float* cols;        // the pass's columns (PASS layout)
  const uint4* cand;
  const int32_t* cand_cnt;
  const float* qeps;        // [M * 32]
  const int32_t* in_rows;   // [na][3]
  int32_t* viol;            // [0] += rows with a cosine outside its bracket, [1] += rows checked (count_checked)
  int32_t* flag;            // |= 2: a candidate buffer overflowed (the host redoes the pass)
  int32_t* cand_total;      // += the candidates this analogy refined
  int cap, d, k, count_checked;
  const int32_t* ids;
  int32_t* out_ids;         // [na][k] of the pass
  double* out_score;
};
template <int M>
__global__ __launch_bounds__(64 * AN_RW) void an_refine_kernel(AnRefineArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);                                                    // [M][d]
  u64* lo = reinterpret_cast<u64*>(smem + (((size_t)M * a.d * 4 + 15) & ~(size_t)15));          // [AN_RW][AN_SLOTS]
  uint32_t* lr = reinterpret_cast<uint32_t*>(lo + AN_RW * AN_SLOTS);
  __shared__ int cnts[AN_RW];
  const int j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = a.d;
  for (int i = threadIdx.x; i < M * d; i += 64 * AN_RW) {
    const int m = i / d, dim = i - m * d;
    qs[i] = a.cols[((size_t)m * AN_PASS + j) * d + dim];
  }
  __syncthreads();
  int cnt = a.cand_cnt[j];
  if (cnt > a.cap) { if (threadIdx.x == 0) atomicOr(a.flag, 2); return; }
  float eps[M];
#pragma unroll
  for (int m = 0; m < M; ++m) eps[m] = a.qeps[m * 32 + j];
  const int32_t x1 = a.in_rows[j * 3 + 0], x2 = a.in_rows[j * 3 + 1], x3 = a.in_rows[j * 3 + 2];
  AnTop top;
  top.init(lo + wave * AN_SLOTS, lr + wave * AN_SLOTS, a.k);
  int viol = 0;
  for (int base = wave * 64; base < cnt; base += 64 * AN_RW) {
    const bool v = base + lane < cnt;
    const uint4 c = a.cand[(size_t)j * a.cap + (v ? base + lane : 0)];
    const float4* x = reinterpret_cast<const float4*>(a.rows + (size_t)c.x * d);
    float acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] = 0.0f;
    int i = 0;
    for (; i + 16 <= d; i += 16) {      // core_functions.c:77: scalar += v1[i] * v2[i], i ascending, each operation rounded
      float4 xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) xv[u] = x[(i >> 2) + u];
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 qv = *reinterpret_cast<const float4*>(qs + m * d + i + 4 * u);
          acc[m] = acc[m] + qv.x * xv[u].x; acc[m] = acc[m] + qv.y * xv[u].y;
          acc[m] = acc[m] + qv.z * xv[u].z; acc[m] = acc[m] + qv.w * xv[u].w;
        }
    }
    for (; i < d; ++i) {
      const float xi = reinterpret_cast<const float*>(x)[i];
#pragma unroll
      for (int m = 0; m < M; ++m) acc[m] = acc[m] + qs[m * d + i] * xi;
    }
    const float ap[3] = {__uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w)};
    bool out = false;
#pragma unroll
    for (int m = 0; m < M; ++m) out = out || (ap[m] == ap[m] && acc[m] == acc[m] && !(__builtin_fabsf(acc[m] - ap[m]) <= eps[m]));
    if (v && out) ++viol;
    const double s = (M == 1) ? (double)acc[0] : an_mul_score(acc[0], acc[M > 1 ? 1 : 0], acc[M > 2 ? 2 : 0]);
    const bool input = (int32_t)c.x == x1 || (int32_t)c.x == x2 || (int32_t)c.x == x3;
    top.push(an_ord(s), c.x, v && !input);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) viol += __shfl_xor(viol, o, 64);
  if (lane == 0 && viol) atomicAdd(a.viol + 0, viol);
  if (a.count_checked && threadIdx.x == 0) atomicAdd(a.viol + 1, cnt);
  if (threadIdx.x == 0) atomicAdd(a.cand_total, cnt);
  if (lane == 0) cnts[wave] = top.cnt;
  __syncthreads();
  if (wave != 0) return;
  an_absorb(top, lo, lr, cnts, AN_RW);
  for (int r = lane; r < a.k; r += 64) {
    const bool v = r < top.cnt;
    a.out_ids[(size_t)j * a.k + r] = v ? a.ids[top.row[r]] : -1;
    a.out_score[(size_t)j * a.k + r] = v ? an_unord(top.ord[r]) : -__builtin_huge_val();
  }
}

static inline size_t an_refine_lds(int M, int d) {
  return (((size_t)M * d * 4 + 15) & ~(size_t)15) + (size_t)AN_RW * AN_SLOTS * (sizeof(u64) + sizeof(uint32_t));
}
template <int M, int AT>
static inline size_t an_scan_lds(int d) {
  return (((size_t)d * M * AT * 4 + 15) & ~(size_t)15) + (size_t)AN_WAVES * AT * AN_SLOTS * (sizeof(u64) + sizeof(uint32_t));
}

template <int AT>
static inline size_t an_pair_lds(int d) {
  return (((size_t)d * 2 * AT * 4 + 15) & ~(size_t)15) + (size_t)AN_WAVES * AT * AN_SLOTS * (sizeof(u64) + sizeof(uint32_t));
}

}  // namespace freddy
