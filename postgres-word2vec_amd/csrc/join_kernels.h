// join_kernels.h -- the device side of the kNN-join (join.h has the split of work) but for the traversal (join_traverse.h): the
// front kernels, the target-list kernels, and join_query_kernel with its arguments (JoinArgs) and LDS layout (JOIN_LDS_ARRAYS).
#pragma once

#include "dot_chain.h"   // row_of_id
#include "join_index.h"

namespace freddy {

// Cell lists of the (few) queries whose traversal the host had to do (equal keys: the reference's heap order is history-dependent)
// into the rows the device traversal writes for everybody else -- row q of qcells[Q][cells], qcell_cnt[q] -- so that ONE join
// launch serves all queries of a round.  rows: [n][1 + cells] in mapped host memory (count, cells).
__global__ __launch_bounds__(256) void join_fb_rows_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ scan_q,
                                                          int32_t* __restrict__ qcells, int32_t* __restrict__ qcell_cnt, int cells) {
  const int x = blockIdx.x, q = scan_q[x];
  const int32_t* r = rows + (size_t)x * (cells + 1);
  const int n = r[0];
  if (threadIdx.x == 0) qcell_cnt[q] = n;
  for (int i = threadIdx.x; i < n; i += 256) qcells[(size_t)q * cells + i] = r[1 + i];
}
__global__ __launch_bounds__(256) void join_copy_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------
// sub-distances of every query to the multi-index centroids       index_utils.c:297-305
// out[q][pos][code]; lane <-> code (coalesced centroid reads), query half-vector via scalar cache
// ---------------------------------------------------------------------------------------
// copy_out != NULL: `queries` is the pinned staging block (mapped host memory) -- the workgroup pulls its half vector over
// PCIe ONCE (16-byte loads), keeps it in LDS, and also writes it to the device copy the join kernel reads: the query batch
// crosses PCIe inside this kernel, piece by piece behind the host's staging copy (no separate copy kernels, and the
// sub-distances of a piece are done when its bytes have arrived).  q0: first query of the launch.
__global__ __launch_bounds__(64) void sub_dist_kernel(const float* __restrict__ queries,
                                                     const float* __restrict__ coarseT,
                                                     float* __restrict__ out, int d, int Kc,
                                                     float* __restrict__ copy_out = nullptr, int q0 = 0) {
  __shared__ __attribute__((aligned(16))) float qh[512];
  const int q = q0 + blockIdx.x, pos = blockIdx.y;
  const int half = d / 2;
  const float* qv = queries + (size_t)q * d + (size_t)pos * half;
  const bool staged = copy_out != nullptr && half <= 512;
  if (staged) {
    if ((half & 3) == 0 && (((size_t)q * d + (size_t)pos * half) & 3) == 0) {
      const int n4 = half >> 2;
      for (int i = threadIdx.x; i < n4; i += 64) {
        const float4 v = reinterpret_cast<const float4*>(qv)[i];
        reinterpret_cast<float4*>(qh)[i] = v;
        reinterpret_cast<float4*>(copy_out + (size_t)q * d + (size_t)pos * half)[i] = v;
      }
    } else {
      for (int i = threadIdx.x; i < half; i += 64) { const float v = qv[i]; qh[i] = v; copy_out[(size_t)q * d + (size_t)pos * half + i] = v; }
    }
    __syncthreads();
    qv = qh;
  }
  for (int c = threadIdx.x; c < Kc; c += 64) {
    float acc = 0.0f;
    // (the sum is sequential -- squareDistance's order -- but the loads are not: one at a time, each waited for, the kernel was
    //  150 dependent round trips long: 53 us for 5 000 queries; fifteen in flight per batch)
    constexpr int NB = 15;
    int i = 0;
    for (; i + NB <= half; i += NB) {
      float cv[NB], qq[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) { cv[u] = coarseT[((size_t)pos * half + i + u) * Kc + c]; qq[u] = qv[i + u]; }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const float t = qq[u] - cv[u];
        const float p = t * t;
        acc = acc + p;
      }
    }
    for (; i < half; ++i) {
      const float t = qv[i] - coarseT[((size_t)pos * half + i) * Kc + c];
      const float p = t * t;
      acc = acc + p;
    }
    out[((size_t)q * 2 + pos) * Kc + c] = acc;
  }
}

// The front of a join whose queries are rows of a device table (freddy_gpu_knn_join_ids; JoinRun::front_rows): grid (nq, 2), 64
// lanes, as sub_dist_kernel.  rows: [nq] row numbers in mapped host memory -- the workgroup reads its own once (the index is
// wave-uniform: one scalar load over PCIe, 4 bytes instead of sub_dist_kernel's half vector); a row outside [0, n_table) gives
// zeros, as query_gather_kernel does.  The half row goes from table + row * d + pos * half into LDS and into copy_out[q] (the
// block the join kernel reads), with 16-byte loads where half and the offset allow them; then sub_dist_kernel's loop, statement for
// statement, over the LDS copy: the bits of `out` are sub_dist_kernel's over the same vectors.  half <= 512 (the launcher's part).
__global__ __launch_bounds__(64) void sub_dist_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ rows, int64_t n_table,
                                                          const float* __restrict__ coarseT, float* __restrict__ out, int d, int Kc,
                                                          float* __restrict__ copy_out) {
  __shared__ __attribute__((aligned(16))) float qh[512];
  const int q = blockIdx.x, pos = blockIdx.y;
  const int half = d / 2;
  const int64_t row = rows[q];
  const bool known = row >= 0 && row < n_table;
  const size_t src = (size_t)(known ? row : 0) * d + (size_t)pos * half;
  float* dst = copy_out + (size_t)q * d + (size_t)pos * half;
  if ((half & 3) == 0 && (src & 3) == 0) {   // (half % 4 == 0 makes d a multiple of 8: dst is 16-byte aligned as well)
    const int n4 = half >> 2;
    for (int i = threadIdx.x; i < n4; i += 64) {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (known) v = reinterpret_cast<const float4*>(table + src)[i];
      reinterpret_cast<float4*>(qh)[i] = v;
      reinterpret_cast<float4*>(dst)[i] = v;
    }
  } else {
    for (int i = threadIdx.x; i < half; i += 64) { const float v = known ? table[src + i] : 0.0f; qh[i] = v; dst[i] = v; }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < Kc; c += 64) {
    float acc = 0.0f;
    constexpr int NB = 15;   // (loads in flight per batch: sub_dist_kernel)
    int i = 0;
    for (; i + NB <= half; i += NB) {
      float cv[NB], qq[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) { cv[u] = coarseT[((size_t)pos * half + i + u) * Kc + c]; qq[u] = qh[i + u]; }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const float t = qq[u] - cv[u];
        const float p = t * t;
        acc = acc + p;
      }
    }
    for (; i < half; ++i) {
      const float t = qh[i] - coarseT[((size_t)pos * half + i) * Kc + c];
      const float p = t * t;
      acc = acc + p;
    }
    out[((size_t)q * 2 + pos) * Kc + c] = acc;
  }
}

// Stable ascending order of one side's Kc sub-distances (index_utils.c:306-320 sorts each position's
// distances; equal distances keep their code order): key = (distance bits << 32 | code), one wave per
// (query, position).  Kc <= 64 * V.
template <int V>
__global__ __launch_bounds__(64) void side_sort_kernel(const float* __restrict__ sub, u64* __restrict__ sorted, int Kc,
                                                      const int32_t* __restrict__ only = nullptr) {
  // (query * 2 + position); `only`: the queries to sort (a handful that the device traversal handed back)
  const size_t row = only ? (size_t)only[blockIdx.x >> 1] * 2 + (blockIdx.x & 1) : (size_t)blockIdx.x;
  const int lane = threadIdx.x;
  u64 key[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = v * 64 + lane;
    key[v] = (c < Kc) ? make_key(sub[row * Kc + c], (uint32_t)c) : KEY_INF;
  }
  wave_sort_full<V>(key);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = v * 64 + lane;
    if (c < Kc) sorted[row * Kc + c] = (key[v] << 32) | (key[v] >> 32);   // memory layout of JoinSide {float dist; int code}
  }
}

// "fq.id IN (targets)" on the device: every target id is resolved to its row (ids ascending: affine
// shortcut or binary search), duplicates and unknown ids drop out through a bitmap, the survivors are
// counted per coarse cell, and a second pass scatters them into per-cell buckets.  (Order inside a
// bucket is arbitrary: the join kernel keys every candidate by (distance, row).)
__global__ __launch_bounds__(256) void join_mark_kernel(const int32_t* __restrict__ tids, int n, const int32_t* __restrict__ ids,
                                                       int64_t N, int affine, const int32_t* __restrict__ cell,
                                                       uint32_t* __restrict__ mark, int32_t* __restrict__ win,
                                                       int32_t* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t id = tids[i];
  int64_t r = -1;
  if (affine) {
    const int64_t c = (int64_t)id - ids[0];
    if (c >= 0 && c < N) r = c;
  } else {
    r = row_of_id(ids, N, id);
  }
  int32_t w = -1;
  if (r >= 0) {
    const uint32_t bit = 1u << (r & 31);
    if (!(atomicOr(mark + (r >> 5), bit) & bit)) { w = (int32_t)r; atomicAdd(cnt + cell[r], 1); }
  }
  win[i] = w;
}
__global__ __launch_bounds__(256) void join_offsets_kernel(const int32_t* __restrict__ cnt, int cells, int32_t* __restrict__ off,
                                                          int32_t* __restrict__ fill, int32_t* __restrict__ off_host) {
  __shared__ int scan[256];
  const int tid = threadIdx.x, per = (cells + 255) / 256;
  const int c0 = tid * per, c1 = (c0 + per < cells) ? c0 + per : cells;
  int sum = 0;
  for (int c = c0; c < c1; ++c) sum += cnt[c];
  scan[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = (tid >= o) ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  int run = scan[tid] - sum;
  for (int c = c0; c < c1; ++c) { off[c] = run; fill[c] = run; off_host[c] = run; run += cnt[c]; }   // (off_host: mapped host memory)
  if (tid == 255) { off[cells] = scan[255]; off_host[cells] = scan[255]; }
}
__global__ __launch_bounds__(256) void join_place_kernel(const int32_t* __restrict__ win, int n, const int32_t* __restrict__ cell,
                                                        int32_t* __restrict__ fill, int32_t* __restrict__ trow) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t r = win[i];
  if (r >= 0) trow[atomicAdd(fill + cell[r], 1)] = r;
}

// ---------------------------------------------------------------------------------------
// one workgroup per scanned query
// ---------------------------------------------------------------------------------------
struct JoinArgs {
  const float* queries;       // [Q][d]
  const int32_t* scan_query;  // [n_scan] query index
  const int32_t* qcell_off;   // [n_scan+1] offsets into qcells (host traversal), or NULL:
  const int32_t* qcell_cnt;   // [Q] cells in row q of qcells[Q][qstride] (device traversal)
  int qstride;
  const int32_t* qcells;      // cells probed by each scanned query
  const int32_t* tcell_off;   // [cells+1] target buckets by cell
  const int32_t* trow;        // target rows, ascending inside a bucket
  const int32_t* ids;         // [N]
  const int16_t* codes;       // [N][MP], rows 16-byte aligned
  int MP;
  const float* vectors;       // [N][d]
  const float* cbT;           // [m][S][K]
  int32_t* out_ids;           // [n_scan][k]
  float* out_dist;            // [n_scan][k]
  int d, m, K, S, k, L, method, double_codes;
  // BIG instantiation (more than 1024 candidates: k * pvf or 2k up to 8192): the candidates and, for post verification, their
  // exact distances
  u64* big_keys = nullptr;    // [n_scan][L]
  float* big_exact = nullptr; // [n_scan][L] (method 2 only)
};

// The dynamic LDS of join_query_kernel<V>, array by array in the order they lie: X(element type, name, bytes; every size a
// multiple of 16 but the last).  The kernel carves its pointers with this list and the host sums it (join_lds_bytes), so the
// two cannot drift apart.  16 spare bytes follow the last array; BIG keeps the previous pass's largest key in them.
#define JOIN_LDS_ARRAYS(X, d, lutN, k, V)                                                                             \
  X(float, qv, ((size_t)(d) * 4 + 15) & ~(size_t)15)             /* the query */                                      \
  X(float, lut, ((size_t)(lutN) * 4 + 15) & ~(size_t)15)         /* [m][K] its sub-distances to the codebook */        \
  X(u64, stage, (size_t)JOIN_WAVES * 64 * 8)                     /* per wave: WaveSelect's staging */                  \
  X(u64, lists, (size_t)JOIN_WAVES * 64 * (V) * 8)               /* per wave: its selection; then the candidates */    \
  X(float, exact, ((size_t)64 * (V) * 4 + 15) & ~(size_t)15)     /* post verification's exact distances */             \
  X(float, s_d, ((size_t)(k) * 4 + 15) & ~(size_t)15)            /* [k] the list */                                    \
  X(int32_t, s_id, ((size_t)(k) * 4 + 15) & ~(size_t)15)                                                              \
  X(int32_t, c_start, (size_t)JOIN_CELL_CHUNK * 4)               /* first target slot of a cell of the chunk */        \
  X(int32_t, c_pref, (size_t)(JOIN_CELL_CHUNK + 1) * 4)          /* [chunk + 1] rows before it */
static inline size_t join_lds_bytes(int d, int m, int K, int k, int V) {
  size_t off = 0;
#define JOIN_LDS_COUNT(T, name, bytes) off += bytes;
  JOIN_LDS_ARRAYS(JOIN_LDS_COUNT, d, m * K, k, V)
#undef JOIN_LDS_COUNT
  return off + 16;
}

__device__ __forceinline__ float sqdist_seq(const float* a, const float* __restrict__ b, int n) {
  float acc = 0.0f;                                   // index_utils.c:500-508
  for (int i = 0; i < n; ++i) {
    const float t = a[i] - b[i];
    const float p = t * t;
    acc = acc + p;
  }
  return acc;
}

// the same chain, the vector read with 16-byte loads (a lane walks its own row: a quarter of the load instructions)
__device__ __forceinline__ float sqdist_seq4(const float* a, const float* __restrict__ b, int n) {
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float acc = 0.0f;
  for (int i = 0; i < n; i += 4) {
    const float4 v = b4[i >> 2];
    float t = a[i] - v.x;     float p = t * t; acc = acc + p;
    t = a[i + 1] - v.y; p = t * t; acc = acc + p;
    t = a[i + 2] - v.z; p = t * t; acc = acc + p;
    t = a[i + 3] - v.w; p = t * t; acc = acc + p;
  }
  return acc;
}

// BIG (V = 16; method 2 with 1024 < k * pvf <= 8192, methods 0 / 1 with 1024 < 2k <= 8192): the L smallest (ADC or exact distance,
// row) keys are selected 1024 at a time -- pass p walks the query's candidate rows again and admits only keys above the largest
// key of pass p - 1 (keys are unique: the row is part of them) -- into a list in memory.  Method 2's post verification and
// replay read it there; for methods 0 / 1 the kernel ends with the passes and bigk_replay_kernel (bigk.h) writes the lists.
template <int V, bool BIG = false>
__global__ __launch_bounds__(JOIN_WG) void join_query_kernel(JoinArgs a) {
  static_assert(!BIG || V == 16, "selection passes are 1024 keys wide");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = a.d, m = a.m, K = a.K, S = a.S, k = a.k, L = a.L;
  const int lutN = m * K;
  const int n_codes = a.double_codes ? m / 2 : m;
  size_t off = 0;
#define JOIN_LDS_CARVE(T, name, bytes) T* name = reinterpret_cast<T*>(smem + off); off += bytes;
  JOIN_LDS_ARRAYS(JOIN_LDS_CARVE, d, lutN, k, V)
#undef JOIN_LDS_CARVE
  u64* const s_floor_p = reinterpret_cast<u64*>(smem + ((off + 7) & ~(size_t)7));   // (BIG; inside the 16 spare bytes)

  const int x = blockIdx.x;
  const int q = a.scan_query[x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  for (int i = threadIdx.x; i < d; i += JOIN_WG) qv[i] = a.queries[(size_t)q * d + i];
  __syncthreads();
  if (a.method != FREDDY_METHOD_EXACT) {
    // getPrecomputedDistances, index_utils.c:445-455
    for (int e = threadIdx.x; e < lutN; e += JOIN_WG) {
      const int p = e / K, c = e - p * K;
      float acc = 0.0f;
      for (int i = 0; i < S; ++i) {
        const float t = qv[p * S + i] - a.cbT[((size_t)p * S + i) * K + c];
        const float pr = t * t;
        acc = acc + pr;
      }
      lut[e] = acc;
    }
    __syncthreads();
    // (pair codes -- getPrecomputedDistancesDouble, index_utils.c:457-475: a table of the sums of the two rounded
    // sub-distances, n_codes x K^2 entries -- are NOT tabulated: the scan adds the two entries itself, the same binary32
    // addition the table would hold.  15 x 32^2 floats = 61 KB of LDS per workgroup allowed two workgroups per CU.)
  }
  const float* tab = lut;
  const bool vec4 = (d & 3) == 0;   // (rows of d floats are then 16-byte aligned: hipMalloc'd base, pitch 4 d)

  WaveSelect<V> sel;
  const int c_begin = a.qcell_off ? a.qcell_off[x] : q * a.qstride;
  const int c_end = a.qcell_off ? a.qcell_off[x + 1] : c_begin + a.qcell_cnt[q];
  u64 floor_key = 0;
  const int n_pass = BIG ? (L + 64 * V - 1) / (64 * V) : 1;
  for (int pass = 0; pass < n_pass; ++pass) {
  sel.init(stage + wave * 64, (u64)__float_as_uint(JOIN_MAX_DIST) << 32, BIG ? 64 * V : L);
  // The target rows of the query's cells as ONE index space: a query takes ~40 cells of ~16 target rows each, and a loop
  // "cell by cell, 64 rows at a time" left three quarters of the lanes idle and paid three dependent round trips (cell
  // offsets -> row number -> codes) per cell and wave -- 25-33 us of a 48 us workgroup.  Here the cells' offsets are read
  // once (all together), prefix-summed in LDS, and lane t of a pass takes row t of the concatenation (binary search in the
  // prefix sums): every lane busy, two dependent round trips per 256 rows.
  for (int cb = c_begin; cb < c_end; cb += JOIN_CELL_CHUNK) {
    const int nc = c_end - cb < JOIN_CELL_CHUNK ? c_end - cb : JOIN_CELL_CHUNK;
    __syncthreads();
    for (int i = threadIdx.x; i < nc; i += JOIN_WG) {
      const int cell = a.qcells[cb + i];
      const int r0 = a.tcell_off[cell], r1 = a.tcell_off[cell + 1];
      c_start[i] = r0;
      c_pref[i] = r1 - r0;
    }
    __syncthreads();
    if (wave == 0) {   // exclusive prefix sums: a lane sums its stretch, the wave scans the 64 sums
      const int per = (nc + 63) >> 6, lo = lane * per, hi = lo + per < nc ? lo + per : nc;
      int sum = 0;
      for (int i = lo; i < hi; ++i) sum += c_pref[i];
      int incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
      int run = incl - sum;
      for (int i = lo; i < hi; ++i) { const int c = c_pref[i]; c_pref[i] = run; run += c; }
      if (lane == 63) c_pref[nc] = incl;
    }
    __syncthreads();
    const int T = c_pref[nc];
    for (int base = 0; base < T; base += JOIN_WG) {
      const int t = base + (int)threadIdx.x;
      const bool valid = t < T;
      float dist = 0.0f;
      int32_t row = 0;
      if (valid) {
        int lo = 0, hi = nc;   // the last cell whose prefix is <= t (cells without target rows share a prefix with their successor)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (c_pref[mid] <= t) lo = mid; else hi = mid; }
        row = a.trow[c_start[lo] + (t - c_pref[lo])];
        if (a.method == FREDDY_METHOD_EXACT) {
          dist = vec4 ? sqdist_seq4(qv, a.vectors + (size_t)row * d, d) : sqdist_seq(qv, a.vectors + (size_t)row * d, d);
        } else {
          // the row's codes: MP / 8 loads of 16 bytes (the first four issued together), eight codes each
          const uint4* cd4 = reinterpret_cast<const uint4*>(a.codes + (size_t)row * a.MP);
          const int nch = a.MP >> 3;
          uint4 w4[4];
#pragma unroll
          for (int c8 = 0; c8 < 4; ++c8) w4[c8] = c8 < nch ? cd4[c8] : uint4{0u, 0u, 0u, 0u};
          for (int c0 = 0; c0 < nch; c0 += 4) {
            if (c0 > 0) {
#pragma unroll
              for (int c8 = 0; c8 < 4; ++c8) w4[c8] = c0 + c8 < nch ? cd4[c0 + c8] : uint4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int c8 = 0; c8 < 4; ++c8) {
              const uint32_t ww[4] = {w4[c8].x, w4[c8].y, w4[c8].z, w4[c8].w};
              if (a.double_codes) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {                     // ivpq_search_in.c:446-451 (int16 pair code)
                  const int l = (c0 + c8) * 4 + u;
                  if (l < n_codes) {   // (K^2 <= 32768: the reference's int16 pair code never wraps, join_begin's check)
                    const float pair = tab[(2 * l) * K + (int)(ww[u] & 0xffffu)] + tab[(2 * l + 1) * K + (int)(ww[u] >> 16)];
                    dist = dist + pair;
                  }
                }
              } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) {                     // index_utils.c:1126-1133
                  const int l = (c0 + c8) * 8 + u;
                  if (l < m) dist = dist + tab[K * l + (int)((ww[u >> 1] >> ((u & 1) * 16)) & 0xffffu)];
                }
              }
            }
          }
        }
      }
      const u64 key = make_key(dist, (uint32_t)row);
      sel.push(key, valid && (!BIG || pass == 0 || key > floor_key));
    }
  }
  sel.finish();
  // gather the four waves' lists; wave 0 merges them
#pragma unroll
  for (int v = 0; v < V; ++v) lists[(size_t)wave * 64 * V + v * 64 + lane] = sel.acc[v];
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < JOIN_WAVES; ++w) {
      for (int v = 0; v < V; ++v) {
        const u64 key = lists[(size_t)w * 64 * V + v * 64 + lane];
        if (__ballot(key != KEY_INF) == 0ull) break;   // lists are ascending: the rest is empty too
        wave_topk_absorb_sorted<V>(sel.acc, key);
      }
    }
    if constexpr (BIG) {   // this pass's keys behind the earlier ones: (ADC distance, row) ascending over all passes
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int e = pass * 64 * V + v * 64 + lane;
        if (e < L) a.big_keys[(size_t)x * L + e] = sel.acc[v];
      }
      const u64 top = wave_topk_at<V>(sel.acc, 64 * V - 1);   // KEY_INF: fewer keys than a pass holds -- the rows are exhausted
      if (lane == 0) *s_floor_p = top;
    } else
    if (a.method == FREDDY_METHOD_PQ_PV) {
      // survivors stay in (ADC distance, row) order: that is the order postverify walks them
#pragma unroll
      for (int v = 0; v < V; ++v) lists[v * 64 + lane] = (v * 64 + lane < L) ? sel.acc[v] : KEY_INF;
    } else {
      u64 byp[V];
#pragma unroll
      for (int v = 0; v < V; ++v)
        byp[v] = (sel.acc[v] == KEY_INF || v * 64 + lane >= L) ? KEY_INF : ((sel.acc[v] << 32) | (sel.acc[v] >> 32));
      wave_sort_full<V>(byp);
#pragma unroll
      for (int v = 0; v < V; ++v) lists[v * 64 + lane] = byp[v];
    }
  }
  if constexpr (BIG) {
    __syncthreads();
    floor_key = *s_floor_p;
    if (floor_key == KEY_INF) {   // (the slots of the passes that would follow stay empty)
      for (int e = (pass + 1) * 64 * V + (int)threadIdx.x; e < L; e += JOIN_WG) a.big_keys[(size_t)x * L + e] = KEY_INF;
      break;
    }
  }
  }   // passes
  // (methods 0 / 1 select only: bigk_replay_kernel, launched behind this kernel, turns the query's keys into its list)
  if constexpr (BIG) { if (a.method != FREDDY_METHOD_PQ_PV) return; }
  const u64* const cand = BIG ? a.big_keys + (size_t)x * L : lists;
  float* const exact_d = BIG ? a.big_exact + (size_t)x * L : exact;
  for (int i = threadIdx.x; i < k; i += JOIN_WG) { s_d[i] = JOIN_MAX_DIST; s_id[i] = -1; }
  __syncthreads();
  if (a.method == FREDDY_METHOD_PQ_PV) {
    // postverify, index_utils.c:477-498: exact distance of each of the k*pvf survivors
    // (survivor e on lane e / 4 of wave e % 4: the four waves' loads run side by side)
    for (int e0 = 0; e0 < L; e0 += JOIN_WG) {
      const int e = e0 + (int)(threadIdx.x & 63) * JOIN_WAVES + (int)(threadIdx.x >> 6);
      if (e < L) {
        const u64 c = cand[e];
        exact_d[e] = (c == KEY_INF) ? 0.0f
                   : vec4 ? sqdist_seq4(qv, a.vectors + (size_t)key_pos(c) * d, d) : sqdist_seq(qv, a.vectors + (size_t)key_pos(c) * d, d);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 64 && k <= 64) {
    // insertion replay with the list held one slot per lane (wave_topk.h: wave_list_insert)
    float d_slot = JOIN_MAX_DIST;
    int32_t id_slot = -1;
    float maxd = JOIN_MAX_DIST;
    for (int e = 0; e < L; ++e) {
      const u64 c = cand[e];
      if (c == KEY_INF) break;
      float dist;
      uint32_t row;
      if (a.method == FREDDY_METHOD_PQ_PV) { dist = exact_d[e]; row = key_pos(c); }
      else { dist = __uint_as_float((uint32_t)c); row = (uint32_t)(c >> 32); }
      if (dist < maxd) {
        wave_list_insert(d_slot, id_slot, k, dist, a.ids[row]);
        maxd = wave_list_max(d_slot, k);
      }
    }
    if ((int)threadIdx.x < k) { s_d[threadIdx.x] = d_slot; s_id[threadIdx.x] = id_slot; }
  } else if (threadIdx.x == 0 && k > 64) {
    float maxd = JOIN_MAX_DIST;
    for (int e = 0; e < L; ++e) {
      const u64 c = cand[e];
      if (c == KEY_INF) break;
      float dist;
      uint32_t row;
      if (a.method == FREDDY_METHOD_PQ_PV) { dist = exact_d[e]; row = key_pos(c); }
      else { dist = __uint_as_float((uint32_t)c); row = (uint32_t)(c >> 32); }
      if (dist < maxd) {
        int slot = k - 1;                                // updateTopK, index_utils.c:19-33
        while (slot >= 0 && !(s_d[slot] < dist)) --slot;
        ++slot;
        for (int t = k - 2; t >= slot; --t) { s_d[t + 1] = s_d[t]; s_id[t + 1] = s_id[t]; }
        s_d[slot] = dist;
        s_id[slot] = a.ids[row];
        maxd = s_d[k - 1];
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += JOIN_WG) {
    a.out_ids[(size_t)x * k + i] = s_id[i];
    a.out_dist[(size_t)x * k + i] = s_d[i];
  }
}

}  // namespace freddy
