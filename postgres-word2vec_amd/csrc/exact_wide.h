// exact_wide.h -- the MFMA pass of exact2.h's filter + refine for WIDE rows, 512 < d <= 2048 (option exact_wide).
//
// exf_filter_kernel keeps the whole fragment image of its 64 queries in LDS: 64 d 4 bytes, 128 KiB at d = 512 and more than a
// CU has beyond d = 640.  Everything around it -- the fragment-order copy of the table, exf_prep_kernel, the threshold and
// refine kernels -- is generic in T = ceil(d / 16).  This kernel has the same operands (xf, qfrag, ExfArgs), the same products
// (hi.hi + hi.lo + lo.hi, v_mfma_f32_32x32x16_f16, fp32 accumulators) and the same epilogue; what differs is how the query
// image reaches the matrix cores: it STREAMS through LDS in segments of TS k-steps, two segment buffers per workgroup.
//
//   segment      [NT][TS][hi / lo][64 lanes] x 16 bytes = NT TS 2 KiB  (TS = 8, 64 queries: 32 KiB; two buffers 64 KiB,
//                two workgroups per CU).  Segment s holds k-steps s TS .. s TS + TS - 1 of every tile; the last one may be short.
//   outer round  a wave owns R strips of 32 rows for a whole round and keeps their R NT 16 accumulator registers across the
//                round's segments; the EXF_PF-deep ring of row operands runs on across segment boundaries (TS % EXF_PF == 0:
//                a k-step keeps its ring slot).  The B operands of a k-step are read from LDS once for the wave's R strips.
//   traffic      per round a workgroup takes 8 R 32 d 4 bytes of the table from HBM and re-reads the 64 d 4 bytes of the image
//                from L2 (the image is 512 KiB at most): 1 / (4 R) of the HBM stream.  The table still crosses HBM once per 64 queries.
//
// The order of one segment step g (g counts the segments of all rounds of the workgroup; buffer g & 1 holds segment g):
//
//     fetch   segment g + 1: global -> registers            (all 512 threads; nothing waits for it yet)
//     compute segment g from buffer g & 1                   (waves with a strip: LDS reads + MFMAs)
//     store   registers -> buffer (g + 1) & 1               (the buffer segment g - 1 was read from: every wave finished
//                                                            those reads before it crossed the barrier of step g - 1)
//     barrier                                               (segment g + 1 is visible; buffer g & 1 is released)
//
// ONE barrier per segment is enough because there are two buffers and the store sits between the compute that reads the OTHER
// buffer and the barrier: the buffer being filled is never one a wave may still read.
//
// The number of barriers a wave crosses depends on blockIdx and gridDim alone: `rounds` below is computed from the workgroup's
// first strip, never from the wave's.  A wave whose strips lie beyond the table (n_strips no multiple of 8 R, fewer strips than
// waves, the last round of a grid smaller than the work, SAMPLE mode alike) fetches, stores and crosses every barrier; it skips
// the row loads, the MFMAs and the epilogue only.  A workgroup with no strip at all returns before its first barrier, as one.
// Nothing beyond NT T 2 64 entries of qfrag is read: the k-steps a short last segment lacks are filled with its last real one.
#pragma once
#include "exact2.h"

namespace freddy {

// dynamic LDS of a launch: two segment buffers
static inline size_t exf_wide_lds(int NT, int TS) { return (size_t)2 * NT * TS * 2 * 64 * 16; }
// workgroups: one per 8 R strips, at most `per_cu` per CU (the rounds walk what a smaller grid leaves)
static inline unsigned exf_wide_grid(int n_cus, int64_t rows, int R, int per_cu) {
  const int64_t strips = (rows + 31) / 32;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((strips + 8 * R - 1) / (8 * R), (int64_t)n_cus * per_cu));
}
// workgroups per CU the kernel is compiled for: TS = 8, R = 1 fits 128 registers and 64 KiB twice; the other shapes take a CU each
static constexpr int exf_wide_per_cu(int TS, int R) { return TS == 8 && R == 1 ? 2 : 1; }

typedef uint32_t exw_u4 __attribute__((ext_vector_type(4)));   // a 16-byte entry as a plain vector: the array of them stays in registers
// Segment s of every tile -> registers, entry J of PER per thread (constant indices: the array stays in registers).  The k-steps a
// short last segment lacks repeat its last one (no MFMA reads them): no entry beyond k-step T - 1 is ever loaded.
template <int J, int PER, int TS>
__device__ __forceinline__ void exw_fetch(exw_u4 (&pre)[PER], const exw_u4* __restrict__ src, int tid, int T, int s) {
  constexpr int n = (J * EXF_WG) / (TS * 128), rem0 = (J * EXF_WG) % (TS * 128);   // (tid < EXF_WG divides TS * 128: tile n for the whole workgroup)
  static_assert((TS * 128) % EXF_WG == 0, "a thread's entry J lies in one tile");
  const int rem = rem0 + tid, tl = min(rem >> 7, T - 1 - s * TS);
  pre[J] = src[(n * T + s * TS + tl) * 128 + (rem & 127)];
  if constexpr (J + 1 < PER) exw_fetch<J + 1, PER, TS>(pre, src, tid, T, s);
}
template <int J, int PER>
__device__ __forceinline__ void exw_store(const exw_u4 (&pre)[PER], exw_u4* dst, int tid) {
  dst[tid + J * EXF_WG] = pre[J];
  if constexpr (J + 1 < PER) exw_store<J + 1, PER>(pre, dst, tid);
}

template <int NT, bool SAMPLE, int TS, int R>
__global__ __launch_bounds__(EXF_WG, 2 * exf_wide_per_cu(TS, R)) void exf_wide_filter_kernel(ExfArgs a) {
  constexpr int SEG = NT * TS * 128;        // 16-byte entries of one segment buffer: [NT][TS][2][64]
  constexpr int PER = SEG / EXF_WG;         // entries a thread moves per segment
  constexpr int WAVES = EXF_WG / 64;
  static_assert(TS % EXF_PF == 0, "a k-step keeps its ring slot across segments");
  static_assert(SEG % EXF_WG == 0, "whole entries per thread");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  exw_u4* const buf = reinterpret_cast<exw_u4*>(smem);   // [2][SEG]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, nseg = (T + TS - 1) / TS;
  const int64_t n_strips = (a.n_rows + 31) >> 5;
  // rounds of THIS WORKGROUP (uniform over its waves): round i covers strips (i gridDim.x + blockIdx.x) 8 R .. + 8 R - 1
  const int64_t wg_first = (int64_t)blockIdx.x * (WAVES * R), per_round = (int64_t)gridDim.x * (WAVES * R);
  if (wg_first >= n_strips) return;         // (the whole workgroup, before any barrier)
  const int64_t rounds = (n_strips - wg_first + per_round - 1) / per_round;
  const int64_t G = rounds * nseg;          // segment steps = barriers behind the first one, for every wave alike

  const exw_u4* const src = reinterpret_cast<const exw_u4*>(a.qfrag);
  exw_u4 pre[PER];
  exw_fetch<0, PER, TS>(pre, src, tid, T, 0);
  exw_store<0, PER>(pre, buf, tid);
  __syncthreads();

  const int i_row = lane & 31, g5 = lane >> 5;
  f16acc acc[R][NT];
  h8v ring[R][EXF_PF][2];                   // the strips' operands: [t][hi / lo][64 lanes], EXF_PF k-steps in flight
  const h8v* xs[R];
  bool live[R];                             // (wave-uniform)
  int64_t strip0 = 0;
  auto issue = [&](int r, int slot, int t) __attribute__((always_inline)) {
    ring[r][slot][0] = xs[r][(size_t)(2 * t) * 64];
    ring[r][slot][1] = xs[r][(size_t)(2 * t + 1) * 64];
  };
  int s = 0;
  int64_t round = 0;
  for (int64_t g = 0; g < G; ++g) {
    const bool more = g + 1 < G;
    const int s_next = s + 1 == nseg ? 0 : s + 1;
    if (more) exw_fetch<0, PER, TS>(pre, src, tid, T, s_next);
    if (s == 0) {                           // a round begins: the wave's strips, cleared accumulators, the ring's first loads
      strip0 = wg_first + round * per_round + (int64_t)wave * R;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        live[r] = strip0 + r < n_strips;
        xs[r] = a.xf + (size_t)(live[r] ? (SAMPLE ? (strip0 + r) * a.strip_stride : strip0 + r) : 0) * T * 128 + lane;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[r][n][v] = 0.0f;
        if (live[r]) {
#pragma unroll
          for (int p = 0; p < EXF_PF; ++p) if (p < T) issue(r, p, p);
        }
      }
    }
    if (live[0]) {                          // (strips of a wave are consecutive: no strip 0, no strip at all)
      const h8v* qf = reinterpret_cast<const h8v*>(buf + (size_t)(g & 1) * SEG) + lane;
      const int t_seg = s * TS;
#pragma unroll 1
      for (int tl0 = 0; tl0 < TS; tl0 += EXF_PF)
#pragma unroll
      for (int p = 0; p < EXF_PF; ++p) {
        const int tl = tl0 + p, t = t_seg + tl;
        if (t < T) {
          h8v bh[NT], bl[NT];
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            bh[n] = qf[((n * TS + tl) * 2 + 0) * 64];
            bl[n] = qf[((n * TS + tl) * 2 + 1) * 64];
          }
#pragma unroll
          for (int r = 0; r < R; ++r) {
            if (r == 0 || live[r]) {
              const h8v hi = ring[r][p][0], lo = ring[r][p][1];
              if (t + EXF_PF < T) issue(r, p, t + EXF_PF);
#pragma unroll
              for (int n = 0; n < NT; ++n) {
                acc[r][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi, bh[n], acc[r][n], 0, 0, 0);
                acc[r][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi, bl[n], acc[r][n], 0, 0, 0);
                acc[r][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(lo, bh[n], acc[r][n], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    if (more) exw_store<0, PER>(pre, buf + (size_t)((g + 1) & 1) * SEG, tid);
    __syncthreads();
    if (s == nseg - 1) {                    // the round's last segment: the epilogue of exf_filter_kernel per strip
      // C layout: register v of lane l = row (v & 3) + 8 (v >> 2) + 4 (l >> 5) of the strip, column l & 31
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!live[r]) continue;
        const int64_t strip = strip0 + r;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int q = 32 * n + i_row;
          // (read per round, not kept: the registers go to the segment in flight; the two words stay in cache)
          const float thr = SAMPLE ? 0.0f : a.thr[q], unsc = a.qunscale[q];
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int64_t row = strip * 32 + (v & 3) + 8 * (v >> 2) + 4 * g5;
            if constexpr (SAMPLE) {
              if (row < a.n_rows) a.sample_out[(size_t)q * a.n_rows + row] = acc[r][n][v] * unsc;
            } else {
              if (!(acc[r][n][v] < thr) && row < a.n_rows) {     // (a NaN passes: the refine stage decides)
                const int slot = atomicAdd(a.cand_cnt + q, 1);
                if (slot < a.cap) a.cand[(size_t)q * a.cap + slot] = uint2{(uint32_t)row, __float_as_uint(acc[r][n][v] * unsc)};
              }
            }
          }
        }
      }
      ++round;
    }
    s = s_next;
  }
}

}  // namespace freddy
