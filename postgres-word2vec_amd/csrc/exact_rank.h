// exact_rank.h -- what exact2.h's filter + refine needs for result lists of 33 .. 1024 rows (option exact_filter_k):
//   exf_rank_threshold_kernel   tau = the EXACT k-th largest approximate similarity of the sample, by radix rank selection
//   exf_refine_tree_kernel<V>   the refine stage with a selection V = pick_V(k) registers wide, its sixteen waves' lists met by a tree
// The filter kernels between them (exact2.h, exact_wide.h) do not know k.  exf_threshold_kernel takes the k-th best of the 1024
// lanes' best sample rows: a valid threshold only while k <= 64 (a wave's selection) and a sharp one only while k^2 / 2048 is small.
// The k-th largest value of the sample itself is the tau of exact2.h's argument for any k: k sample rows have a >= tau, hence
// s >= tau - eps, so the k-th largest exact similarity of the table is >= tau - eps and every row that reaches it has a >= tau - 2 eps.
// The selection orders binary32 patterns, where -0 sorts below +0.  Which of the two the k-th place holds does not matter: they are
// numerically equal, tau - 2 eps is the same number for both, and the filter compares numbers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact2.h"

namespace freddy {

// ---- tau by rank selection -------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads per query (exf_threshold_kernel's shape and arguments).  Every value maps to a 32-bit key that
// ascends with the float; three passes over the query's sample (<= 262 144 values = 1 MiB, from cache after the first) count
// the keys whose upper digits match the ones found so far into a histogram over the next digit -- 11, 11 and 10 bits -- and a
// suffix scan over the bins finds the bin that holds rank k and the rank left inside it.  After the third digit the key is known.
// Histogram adds are plain LDS atomics on ONE histogram: the 64 lanes of a wave collide on a bin whichever wave owns the
// histogram, so the adds are atomics either way, and the LDS serves one wave's instruction at a time -- sixteen private copies
// (128 KiB) would spread nothing and cost sixteen times the clearing and one more reduction per pass.  SUBS = 4 (option
// exact_rank_hist = 1: waves w, w + 4, .. share a copy) is the measured alternative: the same time within 2 % (profiles/exact_filter_k_timing.txt).
static constexpr int EXF_RANK_BINS = 2048;
static constexpr int EXF_RANK_MAX_SAMPLE = 262144;
__device__ __forceinline__ uint32_t exf_rank_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending with the float (sim_key's upper word, not inverted)
}
__device__ __forceinline__ float exf_rank_value(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

template <int SUBS>
__global__ __launch_bounds__(64 * EXF_TW) void exf_rank_threshold_kernel(ExfThrArgs a) {
  __shared__ uint32_t hist[SUBS][EXF_RANK_BINS];
  __shared__ uint32_t wave_sum[EXF_TW];
  __shared__ uint32_t found[2];      // the bin of rank k, the rank left inside it
  __shared__ int nan_s;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float NEG_INF = -__builtin_huge_valf();
  if (tid == 0) { a.cand_cnt[q] = 0; nan_s = 0; }
  if (q >= a.nq) { if (tid == 0) a.thr[q] = __builtin_huge_valf(); return; }   // padding columns never pass
  if (a.n_sample < a.k || a.refine_all) { if (tid == 0) a.thr[q] = NEG_INF; return; }   // fewer than k sample rows / refine-all: every row is a candidate
  const float* s = a.sample + (size_t)q * a.n_sample;
  uint32_t* const my_hist = hist[SUBS == 1 ? 0 : wave % SUBS];
  uint32_t prefix = 0, rank = (uint32_t)a.k;      // the key's digits found so far (upper bits), the rank (1-based, from the top) among the keys that share them
  bool nan = false;
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;                       // the digit's lowest bit
    const uint32_t digit_mask = pass == 2 ? 1023u : 2047u;
    const uint32_t above = pass == 0 ? 0u : ~0u << (pass == 1 ? 21 : 10);         // the bits of the digits already found
    for (int i = tid; i < SUBS * EXF_RANK_BINS; i += 64 * EXF_TW) (&hist[0][0])[i] = 0;
    __syncthreads();
    for (int base0 = wave * 64; base0 < a.n_sample; base0 += 64 * EXF_TW * 8) {   // (eight loads in flight)
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int i = base0 + u * 64 * EXF_TW + lane; x[u] = i < a.n_sample ? s[i] : NEG_INF; }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = base0 + u * 64 * EXF_TW + lane;
        if (i < a.n_sample) {
          if (!(x[u] == x[u])) nan = true;
          const uint32_t key = exf_rank_key(x[u]);
          if (((key ^ prefix) & above) == 0) atomicAdd(&my_hist[(key >> shift) & digit_mask], 1u);
        }
      }
    }
    if (pass == 0 && __ballot(nan) != 0ull && lane == 0) nan_s = 1;
    __syncthreads();
    if (nan_s) break;                 // (uniform: read behind the barrier.  A NaN anywhere: every row is a candidate)
    // thread t owns bins 2 t and 2 t + 1; `hi` = keys in the bins above its pair (a suffix sum over the threads: wave, then waves)
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int h = 0; h < SUBS; ++h) { c0 += hist[h][2 * tid]; c1 += hist[h][2 * tid + 1]; }
    uint32_t incl = c0 + c1;          // -> sum over lanes >= this one
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_down((int)incl, o, 64); if (lane + o < 64) incl += t; }
    if (lane == 0) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t hi = incl - (c0 + c1);
    for (int w = wave + 1; w < EXF_TW; ++w) hi += wave_sum[w];
    // exactly one bin has  keys above it < rank <= keys above it + its own  (the pass counted >= rank keys in all)
    if (hi < rank && rank <= hi + c1) { found[0] = 2u * tid + 1; found[1] = rank - hi; }
    else if (hi + c1 < rank && rank <= hi + c1 + c0) { found[0] = 2u * tid; found[1] = rank - hi - c1; }
    __syncthreads();
    prefix |= found[0] << shift;
    rank = found[1];
  }
  if (tid == 0) {
    float thr = NEG_INF;
    if (!nan_s) {
      const float tau = exf_rank_value(prefix);
      // (exf_threshold_kernel's arithmetic, unchanged)
      const float t = tau - 2.0f * a.qeps[q];
      const float tt = t - __builtin_fabsf(t) * 2.4e-7f - 1e-37f;    // (rounded down)
      thr = tt / a.qunscale[q];                                       // exact: a power of two
      thr = thr - __builtin_fabsf(thr) * 2.4e-7f;                     // (scaled products are compared: once more down)
      if (!(thr == thr)) thr = NEG_INF;
    }
    a.thr[q] = thr;
  }
}

// ---- refine for lists wider than one wave's 64 keys -----------------------------------------------------------------------
// exf_refine_kernel's arguments, LDS layout (exf_refine_lds(d, V)), candidate loop and results, with a WaveSelect<V> per wave.
// The sixteen lists then meet through a tree: in round r the waves whose number is a multiple of 2^(r+1) absorb the list of
// wave + 2^r from LDS, 64 keys at a time (ascending: absorption stops at the first batch that is empty or wholly behind the
// absorber's k-th key), and a wave that is read in the next round puts its merged list back first.  Four rounds with a barrier
// between them instead of fifteen serial absorptions of up to V batches by wave 0 -- at V = 16 that is 64 against 240 batches on
// the critical path.  (A kernel of its own, not `if constexpr` inside exf_refine_kernel: that kernel's <1> keeps its instruction
// stream to the letter.)
template <int V>
__global__ __launch_bounds__(64 * EXF_TW) void exf_refine_tree_kernel(ExfRefineArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);                                                     // [d]
  u64* stage = reinterpret_cast<u64*>(smem + (((size_t)a.d * 4 + 15) & ~(size_t)15));             // [EXF_TW][64]
  u64* lists = stage + EXF_TW * 64;                                                               // [EXF_TW][64 * V]
  const int q = blockIdx.x, lane = threadIdx.x & 63, d = a.d;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < d; i += 64 * EXF_TW) qs[i] = a.queries[(size_t)q * d + i];
  __syncthreads();
  int cnt = a.cand_cnt[q];
  if (cnt > a.cap) { if (threadIdx.x == 0) atomicOr(a.viol + 3, 1); cnt = a.cap; }
  const float eps = a.qeps[q];
  WaveSelect<V> sel;
  sel.init(stage + wave * 64, KEY_INF, a.L);
  int viol = 0;
  for (int base = wave * 64; base < cnt; base += 64 * EXF_TW) {
    const bool v = base + lane < cnt;
    const uint2 c = a.cand[(size_t)q * a.cap + (v ? base + lane : 0)];
    const float4* x = reinterpret_cast<const float4*>(a.rows + (size_t)c.x * d);
    float acc = 0.0f;
    int i = 0;
    for (; i + 32 <= d; i += 32) {      // core_functions.c:77: scalar += v1[i] * v2[i], i ascending, each operation rounded
      float4 xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) xv[u] = x[(i >> 2) + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float4 qv = *reinterpret_cast<const float4*>(qs + i + 4 * u);
        acc = acc + qv.x * xv[u].x; acc = acc + qv.y * xv[u].y; acc = acc + qv.z * xv[u].z; acc = acc + qv.w * xv[u].w;
      }
    }
    for (; i < d; ++i) acc = acc + qs[i] * reinterpret_cast<const float*>(x)[i];
    const float ap = __uint_as_float(c.y);
    if (v && ap == ap && acc == acc && !(__builtin_fabsf(acc - ap) <= eps)) ++viol;
    sel.push(sim_key(acc, c.x), v);
  }
  sel.finish();
  u64* const mine = lists + (size_t)wave * 64 * V;
  if (wave & 1) {                       // (round 0 reads the odd waves)
#pragma unroll
    for (int v = 0; v < V; ++v) mine[v * 64 + lane] = sel.acc[v];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) viol += __shfl_xor(viol, o, 64);
  if (lane == 0 && viol) atomicAdd(a.viol + 0, viol);
  if (a.count_checked && threadIdx.x == 0) atomicAdd(a.viol + 1, cnt);
#pragma unroll 1
  for (int step = 1; step < EXF_TW; step <<= 1) {
    __syncthreads();
    if ((wave & (2 * step - 1)) == 0) {
      const u64* theirs = lists + (size_t)(wave + step) * 64 * V;
#pragma unroll 1
      for (int v = 0; v < V; ++v) {
        const u64 key = theirs[v * 64 + lane];
        const u64 first = __shfl(key, 0, 64);                       // the batch's smallest key
        if (first == KEY_INF || first > wave_topk_at<V>(sel.acc, a.L - 1)) break;   // ascending: nothing behind it enters the first L either
        wave_topk_absorb_sorted<V>(sel.acc, key);
      }
    }
    if ((wave & (4 * step - 1)) == 2 * step) {                      // read in the next round
#pragma unroll
      for (int v = 0; v < V; ++v) mine[v * 64 + lane] = sel.acc[v];
    }
  }
  if (wave != 0) return;   // (every wave has passed every barrier: the ones that were read idle through the later rounds)
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int r = v * 64 + lane;
    if (r < a.k) {
      const u64 key = sel.acc[v];
      a.out_ids[(size_t)q * a.k + r] = (key == KEY_INF) ? -1 : a.ids[key_pos(key)];
      a.out_sim[(size_t)q * a.k + r] = (key == KEY_INF) ? -__builtin_huge_valf() : key_sim(key);
    }
  }
  // the call's last workgroup hands the verdict over (every workgroup's overflow flag is in memory before its ticket)
  __threadfence();
  int ticket = 0;
  if (lane == 0) ticket = __hip_atomic_fetch_add(a.arrived, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  ticket = __builtin_amdgcn_readfirstlane(ticket);
  if (ticket == a.total_wgs - 1 && lane == 0) {
    a.flags_out[0] = __hip_atomic_load(a.viol + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.flags_out[1] = __hip_atomic_load(a.qbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.viol[3] = 0; *a.qbad = 0;
    __hip_atomic_store(a.arrived, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace freddy
