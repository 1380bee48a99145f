// tokenize.h -- text vectors from token ids (freddy--0.0.1.sql:1512-1536 tokenize / tokenize_raw): a text is a list of row ids of a
// pinned vector table, its vector the reference's centroid_bytea of the rows, optionally through vec_normalize_bytea.  The texts of a
// call arrive ragged, token_ids[offsets[n_texts]] and offsets[n_texts + 1]; a text holds at most TOK_MAX_LEN ids.
//   tok_resolve_kernel    one lane per (text, token): the id's table row (resolve_row_of against the handle's device id column), -1
//                         where it has none.  Nothing is looked up on the host.
//   tok_rows_kernel       one wave per text: the text's rows into LDS, then its ROW LIST, written back over the front of the text's own
//                         segment, and the list's length to counts[t].  FREDDY_QIDS_TABLE_ORDER: the distinct rows ascending -- a bitonic
//                         sort of the segment padded to a power of two (unknown ids sort behind every row), then neighbours compared;
//                         FREDDY_QIDS_POSITIONAL: the rows that exist, in the given order, duplicates kept.
//   tok_centroid_kernel   one wave per text, lanes across the dimensions (float4 units, or floats).  core_functions.c:371-379:
//                         out[j] = 0, then for the rows i ascending out[j] = out[j] + row_i[j] / (float)n -- a correctly rounded
//                         division and an addition per term, each rounded to binary32, no FMA, never a reciprocal.  The loads of a
//                         row do not depend on the sums: TOK_AHEAD rows are loaded before their terms are added.
//   tok_unit_kernel       vec_normalize_bytea as aa_query_kernel has it: sq = sq + out[j] * out[j] for j ascending, one chain;
//                         len = (float)sqrt((double)sq); out[j] / len.  A chain per LANE: the 64 texts of a workgroup walk their
//                         chains side by side, then the lanes divide the 64 rows elementwise.  For many texts (TOK_UNIT_LANES).
//   tok_unit_wave_kernel  the same with a wave per text and lane 0 walking the chain over the row in LDS.  For fewer texts.
// A text with an empty row list (no ids, or none with a row) has count 0 and a vector of zeros, which the normalisation leaves alone
// (the reference returns a zero-length bytea there); nothing else is special-cased -- a zero centroid of a non-empty list normalises to NaN.
// No matrix cores: every term of every sum is rounded by itself, in the reference's order; there is no product to accumulate.
//
// Bounds.  tok_rows_kernel: the segment of text t is rows[offsets[t] .. offsets[t + 1]); it is read whole into LDS (len <= P <= the
// launch's dynamic LDS, sized for the call's longest text) before position p <= i of it is written.  tok_centroid_kernel reads
// counts[t] <= len entries of the segment, every one a row in [0, N); unit u < U of the row and of the output row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "resolve.h"

namespace freddy {

static constexpr int TOK_MAX_LEN = 4096;   // FREDDY_TOK_MAX_LEN: ids per text (16 KiB of LDS)
static constexpr int TOK_AHEAD = 8;        // rows whose loads are in flight ahead of the adds
// The sum of squares is d dependent adds per text.  tools/tokenize_timing.py (profiles/tokenize_timing.txt, 3 M x 300) timed both forms:
// a wave per text with lane 0 walking the chain takes 8 - 11 us up to 1 024 texts and 236 us at 100 000 (2.4 us per 1 000 texts);
// a chain per lane over the 64 texts of a workgroup takes 44 us at 1 024 texts -- sixteen waves on the whole chip, each walking 300
// strided loads -- and 118 us at 100 000.  The lines cross near 20 000 texts; a wave per text is taken below 16 384 (one workgroup of
// the lane form per CU of a 256-CU chip), the lane form from there on (option tokenize_unit: 0 = this rule, 1 / 2 = one form always).
static constexpr int64_t TOK_UNIT_LANES = 16384;

static __global__ __launch_bounds__(256) void tok_resolve_kernel(const int32_t* __restrict__ ids, int64_t n, const int32_t* __restrict__ vec_ids,
                                                                 int64_t N, int32_t* __restrict__ rows) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) rows[i] = resolve_row_of(vec_ids, N, ids[i]);
}

static inline size_t tok_rows_lds(int max_len) {   // the longest text of the call, padded as the kernel pads it
  int P = 64;
  while (P < max_len) P <<= 1;
  return sizeof(int32_t) * (size_t)P;
}

static __global__ __launch_bounds__(64) void tok_rows_kernel(int32_t* __restrict__ rows, const int64_t* __restrict__ offsets, int n_texts,
                                                             int table_order, int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tok_smem[];
  int32_t* s = reinterpret_cast<int32_t*>(tok_smem);
  constexpr int32_t NONE = 0x7fffffff;   // (no row: a table has fewer than 2^31 - 1 rows)
  const int lane = threadIdx.x;
  for (int t = blockIdx.x; t < n_texts; t += gridDim.x) {
    const int64_t o = offsets[t];
    const int len = (int)(offsets[t + 1] - o);
    int P = 64;
    while (P < len) P <<= 1;
    for (int i = lane; i < P; i += 64) {
      const int32_t r = i < len ? rows[o + i] : -1;
      s[i] = r < 0 ? NONE : r;
    }
    __syncthreads();
    if (table_order && len > 1) {
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = lane; i < P; i += 64) {
            const int p = i ^ j;
            if (p > i) {
              const int32_t a = s[i], b = s[p];
              if ((a > b) == ((i & k) == 0)) { s[i] = b; s[p] = a; }
            }
          }
          __syncthreads();
        }
    }
    int n = 0;
    for (int i0 = 0; i0 < P; i0 += 64) {
      const int i = i0 + lane;
      const int32_t v = s[i];
      const bool keep = v != NONE && (!table_order || i == 0 || s[i - 1] != v);
      const unsigned long long m = __ballot(keep);
      if (keep) rows[o + n + __popcll(m & ((1ull << lane) - 1ull))] = v;
      n += __popcll(m);
    }
    if (lane == 0) counts[t] = n;
    __syncthreads();   // (the next text overwrites s)
  }
}

struct TokArgs {
  const float* table;       // [N][d] the vector handle's row-major copy
  const int32_t* rows;      // the row lists, at the front of every text's segment
  const int64_t* offsets;   // [n_texts + 1]
  const int32_t* counts;    // [n_texts] lengths of the row lists
  const int32_t* sel;       // [n_out] the text of output row q (device or mapped host memory), or NULL: row q is text q
  const float* raw;         // tok_unit: [n_out][d] the centroids
  float* out;               // [n_out][d]
  int64_t n_out;
  int d;
};

__device__ __forceinline__ void tok_add(float& a, const float x, const float fn) { const float q = x / fn; a = a + q; }
__device__ __forceinline__ void tok_add(float4& a, const float4& x, const float fn) {
  tok_add(a.x, x.x, fn); tok_add(a.y, x.y, fn); tok_add(a.z, x.z, fn); tok_add(a.w, x.w, fn);
}
__device__ __forceinline__ void tok_sq(float& sq, const float x) { const float p = x * x; sq = sq + p; }
__device__ __forceinline__ void tok_sq(float& sq, const float4& x) { tok_sq(sq, x.x); tok_sq(sq, x.y); tok_sq(sq, x.z); tok_sq(sq, x.w); }
__device__ __forceinline__ float tok_div(const float x, const float len) { return x / len; }
__device__ __forceinline__ float4 tok_div(const float4& x, const float len) { return make_float4(x.x / len, x.y / len, x.z / len, x.w / len); }

// T = float4 (U = d / 4 units per row) or float (U = d).  A wave takes 128 units of a row at a time, two per lane: the 75 units of
// d = 300 in one walk over the rows.
template <class T>
static __global__ __launch_bounds__(256) void tok_centroid_kernel(TokArgs a, uint32_t U) {
  const uint32_t lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  const T* __restrict__ table = reinterpret_cast<const T*>(a.table);
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < a.n_out; q += stride) {
    const int64_t t = a.sel ? (int64_t)a.sel[q] : q;
    const int32_t* __restrict__ r = a.rows + a.offsets[t];
    const int n = a.counts[t];
    const float fn = (float)n;
    for (uint32_t u0 = 0; u0 < U; u0 += 128) {
      const uint32_t ua = u0 + lane, ub = ua + 64;
      const bool ha = ua < U, hb = ub < U;
      T sa{}, sb{};
      for (int i = 0; i < n; i += TOK_AHEAD) {
        T va[TOK_AHEAD] = {}, vb[TOK_AHEAD] = {};
#pragma unroll
        for (int j = 0; j < TOK_AHEAD; ++j)
          if (i + j < n) {
            const T* __restrict__ row = table + (size_t)r[i + j] * U;
            if (ha) va[j] = row[ua];
            if (hb) vb[j] = row[ub];
          }
#pragma unroll
        for (int j = 0; j < TOK_AHEAD; ++j)
          if (i + j < n) {
            if (ha) tok_add(sa, va[j], fn);
            if (hb) tok_add(sb, vb[j], fn);
          }
      }
      if (ha) out[(size_t)q * U + ua] = sa;
      if (hb) out[(size_t)q * U + ub] = sb;
    }
  }
}

// 64 output rows per workgroup, a chain per lane; then the lanes across the units of the 64 rows.
template <class T>
static __global__ __launch_bounds__(64) void tok_unit_kernel(TokArgs a, uint32_t U) {
  __shared__ float len_s[64];
  __shared__ int live_s[64];
  const uint32_t lane = threadIdx.x;
  const T* __restrict__ raw = reinterpret_cast<const T*>(a.raw);
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  const int64_t n_blocks = (a.n_out + 63) / 64;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t q = b * 64 + lane;
    int live = 0;
    float len = 0.0f;
    if (q < a.n_out) {
      const int64_t t = a.sel ? (int64_t)a.sel[q] : q;
      live = a.counts[t] > 0;
      if (live) {
        const T* __restrict__ v = raw + (size_t)q * U;
        float sq = 0.0f;
        for (uint32_t u = 0; u < U; ++u) tok_sq(sq, v[u]);   // core_functions.c:255-257
        len = (float)sqrt((double)sq);
      }
    }
    len_s[lane] = len;
    live_s[lane] = live;
    __syncthreads();
    const int64_t rows_here = (a.n_out - b * 64 < 64) ? a.n_out - b * 64 : 64;
    const uint32_t total = (uint32_t)rows_here * U;
    const size_t base = (size_t)b * 64 * U;
    for (uint32_t i = lane; i < total; i += 64) {
      const uint32_t ql = i / U;
      const T v = raw[base + i];
      out[base + i] = live_s[ql] ? tok_div(v, len_s[ql]) : v;
    }
    __syncthreads();
  }
}

static inline size_t tok_unit_wave_lds(int d) { return sizeof(float) * (size_t)d; }
static __global__ __launch_bounds__(64) void tok_unit_wave_kernel(TokArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tok_smem[];
  float* rs = reinterpret_cast<float*>(tok_smem);   // [d] the centroid
  __shared__ float len_s;
  const int lane = threadIdx.x, d = a.d;
  for (int64_t q = blockIdx.x; q < a.n_out; q += gridDim.x) {
    const int64_t t = a.sel ? (int64_t)a.sel[q] : q;
    const bool live = a.counts[t] > 0;
    const float* __restrict__ v = a.raw + (size_t)q * d;
    float* __restrict__ out = a.out + (size_t)q * d;
    for (int i = lane; i < d; i += 64) rs[i] = v[i];
    __syncthreads();
    if (lane == 0) {
      float sq = 0.0f;
      if (live)
        for (int i = 0; i < d; ++i) tok_sq(sq, rs[i]);
      len_s = (float)sqrt((double)sq);
    }
    __syncthreads();
    const float len = len_s;
    for (int i = lane; i < d; i += 64) out[i] = live ? rs[i] / len : rs[i];
    __syncthreads();
  }
}

}  // namespace freddy
