// cluster.h -- what generic_cluster (freddy--0.0.1.sql:1086-1209) does between two assignment steps, on the device, so that the
// whole k-means of cluster_exact / cluster_pq is one call (freddy_gpu_cluster, cluster.hip; the contract: include/freddy_gpu.h):
//
//   cluster_init_kernel    once per call.  One lane per position: the row of its token id in the vector handle (binary search over
//       the handle's ascending device ids, row_of_id), clusters[i] = 0, and the smallest position whose id has no row into the
//       flag word (an unsigned atomic minimum; the word starts at 0xffffffff).  kc further workgroups, one per centroid: the row of
//       token pick(n, draws[I]) copied into centroid I, lens[I] = 0.  (That workgroup resolves its own id: nothing in this kernel
//       reads what another workgroup wrote.)
//   cluster_apply_kernel   once per round, behind the assign kernel.  One lane per position, eight positions per thread (2048 per
//       workgroup): a claimed position takes its cluster, and the clusters' lengths are counted with integer atomics -- per workgroup
//       in LDS while kc fits 1024 counters (one global add per cluster and workgroup instead of one per position), straight in
//       memory beyond.  Integer sums do not depend on their order.  A position no centroid claims keeps its cluster: a member that
//       `lens` does not count.  With kc <= 1024 the workgroup also leaves the MEMBERS of every cluster among its 2048 positions
//       (blk_members[kc][n / 2048]: kc * n / 512 bytes, at most half of one of the call's n-entry arrays).
//   cluster_sample_kernel  once per round but the last.  One workgroup per cluster, kmeans_update_kernel's walk (kernels.h): the ten
//       ranks pick(lens[I], draw) first, then clusters[] in index order, 8 x 256 positions per step -- per wave and 256 positions a
//       ballot; the 32 counts of a step through LDS (two buffers, so one barrier per step); where a rank falls into the step, the
//       lane that holds the rank-th set bit records its position.  The plain walk (kc > 1024, n <= 32768, or option cluster_walk = 1) takes the
//       steps from position 0 and ends behind the largest rank: 4 n bytes per cluster, one workgroup's latency per step.  With the
//       apply kernel's counts the walk has two levels: a running sum over the cluster's n / 2048 counts names the step of every
//       rank, and only those (at most ten, each once) steps are taken.  Then the centroid, one
//       thread per dimension, the samples in draw order: c = 0; c = c + (row[j] / (float)ns) -- binary32, the division the correctly
//       rounded one (centroid_bytea, core_functions.c:371-379).  lens[I] = 0 for the next round.  A cluster with lens == 0 returns at
//       once: its centroid stays, its ten draws are skipped by position (the draws of (round, cluster) are a closed form).
//
// Nothing here synchronises with the host; the kernels of a call are ordered by the stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assign.h"
#include "freddy_pick.h"
#include "wave_topk.h"

namespace freddy {

static constexpr int CL_WG = 256;
static constexpr int CL_SUB = 8;            // ballots per wave and step of the sample kernel's walk: 8 x 256 positions per step
static constexpr int CL_SAMPLES = 10;       // draws per cluster and round
static constexpr int CL_HIST = 1024;        // clusters whose lengths a workgroup of the apply kernel counts in LDS
static constexpr int CL_APPLY_PT = 8;       // positions per thread of the apply kernel
static constexpr int CL_STEP = CL_SUB * CL_WG;   // positions per step of the walk = per workgroup of the apply kernel (2048)
static_assert(CL_APPLY_PT == CL_SUB, "a workgroup of the apply kernel counts the members of one step of the walk");
static constexpr uint32_t CL_NO_FLAG = 0xffffffffu;

struct ClusterInitArgs {
  const int32_t* token_ids;   // [n]
  const int32_t* vec_ids;     // [N] ascending ids of the vector handle
  const float* rows;          // [N][d]
  const double* draws;        // [kc] the draws of the initial centroids
  int32_t* row_of;            // [n] out
  int32_t* clusters;          // [n] out: 0
  int32_t* lens;              // [kc] out: 0
  float* centroids;           // [kc][d] out
  uint32_t* flag;             // the smallest position without a row
  int64_t N;
  int n, kc, d;
  unsigned pos_blocks;        // workgroups of positions; the kc behind them are the centroids'
};

static __global__ __launch_bounds__(CL_WG) void cluster_init_kernel(ClusterInitArgs a) {
  const int tid = threadIdx.x;
  if (blockIdx.x < a.pos_blocks) {
    const int64_t i = (int64_t)blockIdx.x * CL_WG + tid;
    if (i < a.n) {
      const int32_t r = row_of_id(a.vec_ids, a.N, a.token_ids[i]);
      a.row_of[i] = r;
      a.clusters[i] = 0;
      if (r < 0) atomicMin(a.flag, (uint32_t)i);
    }
    return;
  }
  const int I = (int)(blockIdx.x - a.pos_blocks);
  const int32_t pos = freddy_pick(a.n, a.draws[I]) - 1;
  const int32_t r = row_of_id(a.vec_ids, a.N, a.token_ids[pos]);   // (the same in every lane)
  if (tid == 0) a.lens[I] = 0;
  for (int j = tid; j < a.d; j += CL_WG) a.centroids[(size_t)I * a.d + j] = r >= 0 ? a.rows[(size_t)r * a.d + j] : 0.0f;
}

struct ClusterApplyArgs {
  const int32_t* best;        // [n] 0-based centroid, -1: no centroid claims the position
  int32_t* clusters;          // [n]
  int32_t* lens;              // [kc]
  int32_t* blk_members;       // [kc][n_blk] members of every cluster among the 2048 positions of every workgroup; NULL: not kept (kc > CL_HIST)
  int n, kc, n_blk;
};

static __global__ __launch_bounds__(CL_WG) void cluster_apply_kernel(ClusterApplyArgs a) {
  __shared__ int32_t hist[CL_HIST], members[CL_HIST];
  const int tid = threadIdx.x;
  const bool in_lds = a.kc <= CL_HIST;
  if (in_lds) {
    for (int j = tid; j < a.kc; j += CL_WG) { hist[j] = 0; members[j] = 0; }
    __syncthreads();
  }
  const int64_t i0 = (int64_t)blockIdx.x * CL_STEP + tid;
#pragma unroll
  for (int u = 0; u < CL_APPLY_PT; ++u) {
    const int64_t i = i0 + (int64_t)u * CL_WG;
    if (i >= a.n) continue;
    const int32_t b = a.best[i];
    const bool claimed = b >= 0 && b < a.kc;
    int32_t c = claimed ? b + 1 : a.clusters[i];       // (the cluster the position is a member of from now on, 0: none)
    if (claimed) {
      a.clusters[i] = c;
      if (in_lds) atomicAdd(&hist[b], 1); else atomicAdd(&a.lens[b], 1);
    }
    if (in_lds && a.blk_members && c > 0) atomicAdd(&members[c - 1], 1);
  }
  if (in_lds) {
    __syncthreads();
    for (int j = tid; j < a.kc; j += CL_WG) {
      if (const int32_t c = hist[j]) atomicAdd(&a.lens[j], c);
      if (a.blk_members) a.blk_members[(size_t)j * a.n_blk + blockIdx.x] = members[j];
    }
  }
}

struct ClusterSampleArgs {
  const int32_t* clusters;    // [n] 1-based, 0: never claimed
  const int32_t* row_of;      // [n]
  const float* rows;          // [N][d]
  const double* draws;        // [kc][10] the draws of this round
  const int32_t* blk_members; // [kc][n_blk] of the apply kernel; NULL: the plain walk
  int32_t* lens;              // [kc] read, then cleared
  float* centroids;           // [kc][d]
  int n, d, n_blk;
};

// One step of the walk: positions c0 .. c0 + 2047 in index order, `running` members of the cluster before them.  The lane that holds
// the rank-th member of a rank in (running, running + members of the step] records its position.  Returns the members through the
// step (the same in every thread).  One barrier; cnt is one of two buffers the caller alternates.
__device__ __forceinline__ int32_t cluster_walk_step(const int32_t* __restrict__ clusters, int n, int32_t mine_id, int64_t c0, int32_t running,
                                                     const int32_t (&rank)[CL_SAMPLES], int32_t (*cnt)[4], int32_t* s_pos) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64 mask[CL_SUB];
#pragma unroll
  for (int k = 0; k < CL_SUB; ++k) {
    const int64_t i = c0 + k * CL_WG + tid;
    const bool mine = i < n && clusters[i] == mine_id;
    mask[k] = __ballot(mine);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < CL_SUB; ++k) cnt[k][wave] = __popcll(mask[k]);
  }
  __syncthreads();
  int32_t seg = running, start[CL_SUB];    // members before this wave's 64 positions of sub-chunk k
#pragma unroll
  for (int k = 0; k < CL_SUB; ++k)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave) start[k] = seg;
      seg += cnt[k][w];
    }
  seg = __builtin_amdgcn_readfirstlane(seg);
#pragma unroll
  for (int t = 0; t < CL_SAMPLES; ++t) {
    if (rank[t] <= running || rank[t] > seg) continue;   // (the same in every thread)
#pragma unroll
    for (int k = 0; k < CL_SUB; ++k) {
      const int32_t rel = rank[t] - start[k];            // 1-based among this wave's members of sub-chunk k
      if (rel >= 1 && rel <= __popcll(mask[k]) && ((mask[k] >> lane) & 1ull) && lanes_below(mask[k]) + 1 == rel)
        s_pos[t] = (int32_t)(c0 + k * CL_WG + tid);
    }
  }
  return seg;
}

static __global__ __launch_bounds__(CL_WG) void cluster_sample_kernel(ClusterSampleArgs a) {
  __shared__ int32_t s_cnt[2][CL_SUB][4];
  __shared__ int32_t s_rank[CL_SAMPLES], s_pos[CL_SAMPLES], s_blk[CL_SAMPLES], s_before[CL_SAMPLES];
  __shared__ int32_t s_wave[2][4];
  const int I = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t len = a.lens[I];
  if (len == 0) return;                      // (the whole workgroup) the centroid stays
  if (tid < CL_SAMPLES) {
    s_rank[tid] = freddy_pick(len, a.draws[(size_t)I * CL_SAMPLES + tid]);
    s_pos[tid] = -1;
    s_blk[tid] = -1;
  }
  __syncthreads();                           // (every thread has read lens[I])
  if (tid == 0) a.lens[I] = 0;
  int32_t rank[CL_SAMPLES], maxrank = 0;
#pragma unroll
  for (int t = 0; t < CL_SAMPLES; ++t) {
    rank[t] = __builtin_amdgcn_readfirstlane(s_rank[t]);
    maxrank = rank[t] > maxrank ? rank[t] : maxrank;
  }
  const int32_t mine_id = I + 1;
  int buf = 0;
  if (a.blk_members) {
    // two levels: the apply kernel left the members of this cluster per 2048 positions; their running sum names the step of every
    // rank, and only those steps are walked
    const int32_t* cnt = a.blk_members + (size_t)I * a.n_blk;
    int32_t running = 0;
    for (int b0 = 0; b0 < a.n_blk && running < maxrank; b0 += CL_WG, buf ^= 1) {
      const int32_t c = b0 + tid < a.n_blk ? cnt[b0 + tid] : 0;
      int32_t incl = c;                      // inclusive sum over the wave, then over the waves
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (lane == 63) s_wave[buf][wave] = incl;
      __syncthreads();
      int32_t before = running, total = running;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) before += s_wave[buf][w];
        total += s_wave[buf][w];
      }
      const int32_t hi = before + incl, lo = hi - c;     // this block holds the members lo + 1 .. hi
#pragma unroll
      for (int t = 0; t < CL_SAMPLES; ++t)
        if (rank[t] > lo && rank[t] <= hi) { s_blk[t] = b0 + tid; s_before[t] = lo; }
      running = __builtin_amdgcn_readfirstlane(total);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < CL_SAMPLES; ++t) {
      const int32_t blk = __builtin_amdgcn_readfirstlane(s_blk[t]);
      bool walked = blk < 0;                 // (a rank beyond the members) -- or a step an earlier rank took: it recorded every rank it holds
#pragma unroll
      for (int u = 0; u < CL_SAMPLES; ++u)
        if (u < t && __builtin_amdgcn_readfirstlane(s_blk[u]) == blk) walked = true;
      if (walked) continue;                  // (the whole workgroup)
      (void)cluster_walk_step(a.clusters, a.n, mine_id, (int64_t)blk * CL_STEP, __builtin_amdgcn_readfirstlane(s_before[t]), rank, s_cnt[buf], s_pos);
      buf ^= 1;
    }
  } else {
    int32_t running = 0;                     // members before this step
    for (int64_t c0 = 0; c0 < a.n && running < maxrank; c0 += CL_STEP, buf ^= 1)
      running = cluster_walk_step(a.clusters, a.n, mine_id, c0, running, rank, s_cnt[buf], s_pos);
  }
  __syncthreads();
  int32_t r[CL_SAMPLES];
  int ns = 0;
#pragma unroll
  for (int t = 0; t < CL_SAMPLES; ++t) {     // (a rank beyond the members vanishes; so does a member without a row, which only a refused call has)
    const int32_t p = s_pos[t];
    r[t] = p >= 0 ? a.row_of[p] : -1;
    if (r[t] >= 0) ++ns;
  }
  if (ns == 0) return;
  const float fn = (float)ns;
  for (int j = tid; j < a.d; j += CL_WG) {
    float c = 0.0f;
#pragma unroll
    for (int t = 0; t < CL_SAMPLES; ++t)
      if (r[t] >= 0) {
        const float q = a.rows[(size_t)r[t] * a.d + j] / fn;   // centroid_bytea: output[j] += data[i][j] / (float) n
        c = c + q;
      }
    a.centroids[(size_t)I * a.d + j] = c;
  }
}

}  // namespace freddy
